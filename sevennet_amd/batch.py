"""Batched graph build: many structures in one `Graph` for one `HipForceEngine.compute` call.

The reference collates many systems into one batched graph (sevenn/torchsim.py:183-292) and reduces energies and virials
per graph (AtomReduce, sevenn/nn/linear.py:127-141; ForceStressOutputFromEdge, sevenn/nn/force_output.py:213-228).  Edges
never cross systems, so the concatenation of B disjoint graphs is itself a valid `Graph`; `Graph.seg_ptr` marks where each
system's atoms start, and the engine then reports `energy_per_system[B]` and `virial_per_system[B,6]` beside the totals.

Graph build: systems of at most `BATCH_MAX_ATOMS` atoms go through ONE batched neighbor-list kernel pair (snet_batch.hip:
one count launch, one scan, one fill launch, one device->host sync for the edge total).  Larger systems take the device
cell list and cells too thin for either device list (a periodic height under 1/64 of the cutoff) the host list -- exactly
what `SevenNetCalculator.compute` does for them -- and `concat_graphs` splices them in.  Results keep the caller's order.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .engine import Graph, build_graph, species_row_lists

# systems above this many atoms use the cell list: the batched kernel is O(n_s^2) per system ("Batched evaluation")
BATCH_MAX_ATOMS = 2048
_MAX_IMAGE_REACH = 64.0   # rc / h_k beyond which a periodic axis goes to the host list (as snet_nl_grid)


def _as_host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().astype(dtype)
    return np.asarray(x, dtype)


def to_device(a, dtype, dev) -> torch.Tensor:
    """a host array as a tensor of `dtype` on `dev`"""
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev, dtype)


def device_positions(positions, dev) -> torch.Tensor:
    """positions (a tensor anywhere, or a host array) as fp64 [N,3] on `dev`.  A tensor that is that already comes back itself:
    who writes to the result clones it first."""
    return (positions.to(dev, torch.float64) if isinstance(positions, torch.Tensor)
            else torch.as_tensor(np.ascontiguousarray(positions, np.float64)).to(dev)).reshape(-1, 3)


def _pad_cells(cells: np.ndarray, pbcs: np.ndarray, cutoff: float) -> np.ndarray:
    """cells[B,3,3] with the zero rows of open axes replaced by a lattice vector along that axis (dataload.py:37-48; the edge
    set does not depend on its length, see snet_batch.hip)"""
    out = cells.copy()
    zero = (np.linalg.norm(out, axis=2) < 1e-12) & ~pbcs
    b, k = np.nonzero(zero)
    out[b, k, :] = 0.0
    out[b, k, k] = 5.0 * cutoff
    return out


def classify_systems(n_atoms: np.ndarray, cells: np.ndarray, pbcs: np.ndarray, cutoff: float,
                     max_atoms: int = BATCH_MAX_ATOMS) -> np.ndarray:
    """per system: 0 = batched kernel, 1 = device cell list (more than `max_atoms` atoms), 2 = host list (a periodic height
    below 1/64 of the cutoff).  A cell that is singular after the open-axis padding raises ValueError: no list can image it."""
    padded = _pad_cells(cells, pbcs, cutoff)
    det = np.linalg.det(padded)
    bad = np.abs(det) <= 1e-12
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError(f'system {b}: singular cell {cells[b].tolist()} (pbc {pbcs[b].tolist()})')
    inv = np.linalg.inv(padded)
    reach = cutoff * np.linalg.norm(inv, axis=1)   # rc / h_k: column k of inv has length 1 / h_k (inv is [B, 3(m), 3(k)])
    thin = ((reach > _MAX_IMAGE_REACH) & pbcs).any(1)
    kind = np.where(n_atoms > max_atoms, 1, 0)
    kind[thin] = 2
    return kind


def _normalize(types, positions, cells, pbcs, n_atoms):
    """-> (types flat, positions flat [N,3], n_atoms int64 [B], cells [B,3,3], pbcs bool [B,3]) with loud validation"""
    if n_atoms is None:   # per-system sequences
        if not isinstance(types, (list, tuple)) or not isinstance(positions, (list, tuple)):
            raise ValueError('pass per-system lists of types and positions, or flat arrays together with n_atoms')
        if len(types) != len(positions):
            raise ValueError(f'{len(types)} type arrays but {len(positions)} position arrays')
        n_atoms = np.array([len(t) for t in types], np.int64)
        n_pos = np.array([len(p) for p in positions], np.int64)
        if not np.array_equal(n_atoms, n_pos):
            b = int(np.nonzero(n_atoms != n_pos)[0][0])
            raise ValueError(f'system {b}: {n_atoms[b]} types but {n_pos[b]} positions')
        if len(types) == 0:
            raise ValueError('empty batch')
        if all(isinstance(p, torch.Tensor) for p in positions):
            positions = torch.cat([p.reshape(-1, 3).to(torch.float64) for p in positions])
        else:
            positions = np.concatenate([_as_host(p, np.float64).reshape(-1, 3) for p in positions])
        if all(isinstance(t, torch.Tensor) for t in types):
            types = torch.cat([t.reshape(-1) for t in types])
        else:
            types = np.concatenate([_as_host(t, np.int64).reshape(-1) for t in types])
    else:
        n_atoms = _as_host(n_atoms, np.int64).reshape(-1)
        if len(n_atoms) == 0:
            raise ValueError('empty batch')
        if int(n_atoms.sum()) != len(types) or len(types) != len(positions):
            raise ValueError(f'n_atoms sums to {int(n_atoms.sum())} but there are {len(types)} types and {len(positions)} positions')
    if (n_atoms <= 0).any():
        raise ValueError(f'system {int(np.nonzero(n_atoms <= 0)[0][0])} has no atoms')
    B = len(n_atoms)
    cells = _as_host(cells, np.float64)
    if cells.size != 9 * B:
        raise ValueError(f'{B} systems but cells of shape {cells.shape}')
    cells = cells.reshape(B, 3, 3)
    pbcs = _as_host(pbcs, bool)
    if pbcs.size == 3:
        pbcs = np.broadcast_to(pbcs.reshape(1, 3), (B, 3))
    if pbcs.size != 3 * B:
        raise ValueError(f'{B} systems but pbc of shape {pbcs.shape}')
    return types, positions, n_atoms, cells, np.ascontiguousarray(pbcs.reshape(B, 3))


def system_of(a_ptr, row: int) -> int:
    """the system that owns flat row `row`, for a_ptr[B+1] = where each system's rows start"""
    return int(np.searchsorted(a_ptr, row, side='right')) - 1


def validate_batch_inputs(types, positions, cells, pbcs, cutoff: float, num_species: int, n_atoms=None,
                          max_atoms: int = BATCH_MAX_ATOMS):
    """Everything `build_batch_graph` would reject, found on the host before the first launch: -> (types int64 [N] on the
    host, positions [N,3] (host array or the caller's tensor), n_atoms [B], cells [B,3,3], pbcs [B,3]).  ValueError names the
    system."""
    types, positions, n_at, cells, pbcs = _normalize(types, positions, cells, pbcs, n_atoms)
    types = _as_host(types, np.int64).reshape(-1)
    a_ptr = np.concatenate([[0], np.cumsum(n_at)])
    bad = (types < 0) | (types >= num_species)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f'system {system_of(a_ptr, i)}: unknown species index {int(types[i])} (the model has {num_species})')
    if not isinstance(positions, torch.Tensor):   # (device tensors are not read back for this)
        fin = np.isfinite(positions).all(1)
        if not fin.all():
            raise ValueError(f'system {system_of(a_ptr, int(np.nonzero(~fin)[0][0]))}: non-finite position')
    if not cutoff > 0:
        raise ValueError(f'cutoff = {cutoff}: a positive cutoff is required')
    classify_systems(n_at, cells, pbcs, cutoff, max_atoms)   # singular cells
    return types, positions, n_at, cells, pbcs


def _batched_neighbors(pos: torch.Tensor, atom_ptr: np.ndarray, cells: np.ndarray, pbcs: np.ndarray, cutoff: float, dev,
                       with_shifts: bool, extra_check: Optional[torch.Tensor] = None, cells_dev: Optional[torch.Tensor] = None):
    """(row_ptr, src, center, edge_vec, shifts) of the systems [atom_ptr[b], atom_ptr[b+1]) of pos (device fp64): one count
    launch, one scan, one fill launch and one device->host sync (the edge total; `extra_check`, a device flag, rides along).
    cells_dev (fp64 [B,9] on the device): the cells the kernels read, instead of an upload of the host `cells`"""
    lib = _lib.load()
    n, B = int(pos.shape[0]), len(atom_ptr) - 1
    st, P = _lib.stream(), _lib.ptr
    ap = torch.as_tensor(atom_ptr.astype(np.int32)).to(dev)
    if cells_dev is None:
        cd = torch.as_tensor(np.ascontiguousarray(cells.reshape(B, 9))).to(dev)
    else:
        _lib.check_device_tensors('build_batch_graph (cells_dev)', pos, [(cells_dev, torch.float64, (B, 9))])
        cd = cells_dev
    pd = torch.as_tensor(pbcs.astype(np.int32)).to(dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.snet_batch_nl_count(P(pos), P(ap), B, P(cd), P(pd), n, float(cutoff), P(count), st), 'snet_batch_nl_count')
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(count.long(), 0)
    if extra_check is None:
        E = int(row_ptr[-1].item())
    else:
        E, bad = torch.stack([row_ptr[-1], extra_check.long()]).cpu().tolist()
        if bad:
            raise ValueError('unknown species index in types')
    if E >= 2 ** 31:
        raise ValueError('more than 2^31 edges')
    row_ptr = row_ptr.to(torch.int32)
    src = torch.empty(E, dtype=torch.int32, device=dev)
    center = torch.empty(E, dtype=torch.int32, device=dev)
    ev = torch.empty(E, 3, dtype=torch.float32, device=dev)
    shifts = torch.empty(E, 3, dtype=torch.int32, device=dev) if with_shifts else None
    if E:
        _lib.check(lib.snet_batch_nl_fill(P(pos), P(ap), B, P(cd), P(pd), n, float(cutoff), P(row_ptr), P(src), P(center), P(ev),
                                          P(shifts), st), 'snet_batch_nl_fill')
    return row_ptr, src, center, ev, shifts, E


def _raw_graph(types, row_ptr, center, src, ev, shifts, E) -> Graph:
    n = int(types.shape[0])
    g = Graph(n, n, E, types, center, src, row_ptr, torch.zeros(n + 1, dtype=torch.int32, device=types.device),
              torch.zeros(0, dtype=torch.int32, device=types.device), ev)
    g.shifts = shifts
    return g


def _slice_graph(g: Graph, a0: int, a1: int, e0: int, e1: int) -> Graph:
    """atoms [a0, a1) and their edges [e0, e1) of a graph without cross edges, renumbered from 0"""
    sh = getattr(g, 'shifts', None)
    return _raw_graph(g.types[a0:a1], g.row_ptr[a0:a1 + 1] - e0, g.center[e0:e1] - a0, g.src[e0:e1] - a0, g.edge_vec[e0:e1],
                      None if sh is None else sh[e0:e1], e1 - e0)


def concat_graphs(graphs: Sequence[Graph], num_species: int = 0, share_pairs: bool = True) -> Graph:
    """One batch Graph from single-system graphs (no ghosts, no halo), in the given order: atoms and edges concatenated with
    offset indices; col_ptr, eperm, the per-species rows (num_species > 0) and the undirected pairs (share_pairs, device
    only) recomputed; `seg_ptr` marks the systems.  Image shifts are kept when every graph has them."""
    if len(graphs) == 0:
        raise ValueError('concat_graphs: no graphs')
    for g in graphs:
        if g.n_total != g.n_local:
            raise ValueError('concat_graphs: graphs with ghost atoms cannot be batched')
    dev = graphs[0].types.device
    n_at = np.array([g.n_local for g in graphs], np.int64)
    n_ed = np.array([g.n_edges for g in graphs], np.int64)
    a_off = np.concatenate([[0], np.cumsum(n_at)])
    e_off = np.concatenate([[0], np.cumsum(n_ed)])
    N, E = int(a_off[-1]), int(e_off[-1])
    if E >= 2 ** 31:
        raise ValueError('more than 2^31 edges')
    types = torch.cat([g.types.to(dev, torch.int32) for g in graphs])
    center = torch.cat([g.center.to(dev).long() + int(a) for g, a in zip(graphs, a_off)]).to(torch.int32)
    src = torch.cat([g.src.to(dev).long() + int(a) for g, a in zip(graphs, a_off)]).to(torch.int32)
    ev = torch.cat([g.edge_vec.to(dev, torch.float32) for g in graphs]).reshape(E, 3)
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev)]
                        + [g.row_ptr[1:].to(dev).long() + int(e) for g, e in zip(graphs, e_off)]).to(torch.int32)
    shifts = [getattr(g, 'shifts', None) for g in graphs]
    sh = torch.cat([s.to(dev, torch.int32) for s in shifts]) if all(s is not None for s in shifts) else None
    return _complete(_raw_graph(types, row_ptr, center.contiguous(), src.contiguous(), ev.contiguous(), sh, E), a_off, num_species,
                     share_pairs)


def _complete(g: Graph, seg_ptr_host: np.ndarray, num_species: int, share_pairs: bool) -> Graph:
    """the source grouping (col_ptr, eperm), per-species rows, system segments and undirected pairs of a raw batch graph"""
    dev, N, E = g.types.device, g.n_local, g.n_edges
    col_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if E:
        col_ptr[1:] = torch.cumsum(torch.bincount(g.src.long(), minlength=N), 0)
        g.eperm = torch.sort(g.src.long(), stable=True).indices.to(torch.int32)
    g.col_ptr = col_ptr.to(torch.int32)
    g.species_rows = species_row_lists(g.types, num_species) if num_species else None
    g.seg_ptr_host = np.asarray(seg_ptr_host, np.int64)
    g.seg_ptr = torch.as_tensor(g.seg_ptr_host.astype(np.int32)).to(dev)
    return g.share_pairs() if share_pairs and dev.type == 'cuda' else g


def _fallback_graph(types_s, pos_s, cell, pbc, cutoff, dev, with_shifts: bool) -> Graph:
    """one system the batched kernel does not take, built as SevenNetCalculator.compute builds it"""
    from .neighbor import neighbor_list
    from .neighbor_gpu import build_graph_gpu, gpu_neighbor_supported
    pos_h = _as_host(pos_s, np.float64)
    if gpu_neighbor_supported(cell, pbc, cutoff, pos_h):
        return build_graph_gpu(types_s, pos_s, cell, cutoff, device=dev, with_shifts=with_shifts, share_pairs=False, pbc=pbc)
    try:
        ei, ev, sh = neighbor_list(pos_h, cell, pbc, cutoff)
    except np.linalg.LinAlgError as e:
        raise ValueError(f'singular cell {np.asarray(cell).tolist()}: no neighbor list handles it') from e
    g = build_graph(types_s, ei, ev, device=dev, share_pairs=False)
    g.shifts = torch.as_tensor(sh).to(dev, torch.int32) if with_shifts else None
    return g


def build_batch_graph(types, positions, cells, pbcs, cutoff: float, num_species: int, *, n_atoms=None, device='cuda:0',
                      species_rows: bool = False, with_shifts: bool = False, share_pairs: bool = True,
                      max_atoms: int = BATCH_MAX_ATOMS, cells_dev: Optional[torch.Tensor] = None) -> Graph:
    """A batch Graph of B systems for HipForceEngine.compute.

    types / positions: per-system sequences (species indices [n_s], positions [n_s,3] in Angstrom), or flat arrays
    [N] / [N,3] together with `n_atoms[B]`; numpy arrays or tensors (device tensors stay on the device).  cells[B,3,3]
    (row vectors) and pbcs[B,3] (or one [3] for all) are small metadata read on the host.  num_species: the model's species
    count (types outside [0, num_species) raise); species_rows: build the per-species row lists an FCTP self-connection
    reads.  Atoms keep the caller's order, so system b is rows [seg_ptr_host[b], seg_ptr_host[b+1]).
    cells_dev: optional fp64 [B,9] tensor on the device with the cells the neighbor kernels read (a cell that moves on the
    device, relax.fire_cell_loop); the host `cells` then only route the systems, all of which must take the batched kernel.
    Raises ValueError on empty systems, mismatched counts, unknown species and singular cells."""
    types, positions, n_at, cells, pbcs = _normalize(types, positions, cells, pbcs, n_atoms)
    dev = torch.device(device)
    B = len(n_at)
    a_ptr = np.concatenate([[0], np.cumsum(n_at)]).astype(np.int64)
    bad_types = None
    if isinstance(types, torch.Tensor):
        ty = types.to(dev, torch.int32)
        bad_types = ((ty < 0) | (ty >= num_species)).any()   # checked with the edge total: no extra sync
    else:
        if ((types < 0) | (types >= num_species)).any():
            raise ValueError(f'unknown species index {int(types[(types < 0) | (types >= num_species)][0])} '
                             f'(the model has {num_species})')
        ty = torch.as_tensor(types.astype(np.int32)).to(dev)
    kind = classify_systems(n_at, cells, pbcs, cutoff, max_atoms)
    if cells_dev is not None and (kind != 0).any():
        b = int(np.nonzero(kind != 0)[0][0])
        raise ValueError(f'system {b}: cells on the device are read by the batched neighbor kernel only, which does not take this '
                         f'system ({"more than " + str(max_atoms) + " atoms" if kind[b] == 1 else "a periodic height below cutoff / 64"})')
    with torch.cuda.device(dev):
        pos = device_positions(positions, dev).contiguous()
        fast = np.nonzero(kind == 0)[0]
        if len(fast) == B:   # every system in the batched kernel: the graph IS its output
            row_ptr, src, center, ev, shifts, E = _batched_neighbors(pos, a_ptr, cells, pbcs, cutoff, dev, with_shifts, bad_types, cells_dev)
            return _complete(_raw_graph(ty, row_ptr, center, src, ev, shifts, E), a_ptr, num_species if species_rows else 0, share_pairs)
        if bad_types is not None and bool(bad_types):
            raise ValueError('unknown species index in types')
        pieces: List[Optional[Graph]] = [None] * B
        if len(fast):   # the batched systems in one build, then cut into systems (one small readback of the row offsets)
            idx = np.concatenate([np.arange(a_ptr[b], a_ptr[b + 1]) for b in fast])
            sub_ptr = np.concatenate([[0], np.cumsum(n_at[fast])])
            sel = torch.as_tensor(idx).to(dev)
            row_ptr, src, center, ev, shifts, E = _batched_neighbors(pos[sel].contiguous(), sub_ptr, cells[fast], pbcs[fast], cutoff,
                                                                     dev, with_shifts)
            gf = _raw_graph(ty[sel], row_ptr, center, src, ev, shifts, E)
            e_at = row_ptr[torch.as_tensor(sub_ptr).to(dev)].cpu().numpy()
            for k, b in enumerate(fast):
                pieces[b] = _slice_graph(gf, int(sub_ptr[k]), int(sub_ptr[k + 1]), int(e_at[k]), int(e_at[k + 1]))
        for b in np.nonzero(kind != 0)[0]:
            a0, a1 = int(a_ptr[b]), int(a_ptr[b + 1])
            pieces[b] = _fallback_graph(ty[a0:a1], pos[a0:a1], cells[b], pbcs[b], cutoff, dev, with_shifts)
        return concat_graphs(pieces, num_species if species_rows else 0, share_pairs)


class BatchForces:
    """The force call of a batched driver (relax.fire_loop, md.md_loop): one `build_batch_graph`, one engine call and one call
    of `extra` per evaluation, and the counters of all of them.

    engine: a HipForceEngine; types int64 [N] on the host, n_atoms [B], cells [B,3,3], pbcs [B,3] as `validate_batch_inputs`
    returns them.  extra: optional callable (positions fp64 [N,3] on the device, seg_ptr int64 [b+1] on the host, ids int64
    [b]: the caller's index of each system of the current batch) -> forces [N,3], or (forces, energy_per_system [b]); numpy or
    torch, on any device.  An `extra` with the attribute `provides_virial = True` (d3.D3DeviceTerm) is also passed
    `cells_dev=` and may return (forces, energies, virial [b,6] in the engine's convention: order xx,yy,zz,xy,yz,zx, stress =
    -virial / volume); the virial of the last evaluation is kept as `virial_extra` (None where there is none), which is where
    relax.fire_cell_loop picks it up.  Nothing touches the device before the first evaluation."""

    def __init__(self, engine, types: np.ndarray, n_atoms: np.ndarray, cells: np.ndarray, pbcs: np.ndarray, cutoff: float,
                 extra: Optional[Callable] = None):
        self.engine, self.types, self.n_atoms, self.cells, self.pbcs = engine, types, np.asarray(n_atoms, np.int64), cells, pbcs
        self.cutoff, self.extra = cutoff, extra
        self.a_ptr = np.concatenate([[0], np.cumsum(self.n_atoms)])
        self.n_force_calls = 0            # engine calls
        self.system_steps_evaluated = 0   # systems in the batch, summed over the engine calls
        self._ids = self._ty = None       # the systems whose species indices are on the device, and those indices
        self.virial_extra = None          # fp64 [b,6] on the device: the virial of `extra` at the last evaluation, if it gave one

    def __call__(self, pos: torch.Tensor, ids=None, want_atomic_virial: bool = False, with_extra: bool = True,
                 cells_dev: Optional[torch.Tensor] = None):
        """Evaluate the systems `ids` (default: all, in the caller's order) at their flat device positions `pos` -> (graph,
        the engine's output, extra forces fp64 [N,3] contiguous on the device or None, extra energies fp64 [b] or None).
        cells_dev: the current cells of those systems (fp64 [b,9] on the device) where they are not the constructor's"""
        eng = self.engine
        dev = eng.dev
        ids = np.arange(len(self.n_atoms)) if ids is None else np.asarray(ids, np.int64)
        if self._ids is None or not np.array_equal(ids, self._ids):   # first call, or the batch has been repacked
            rows = np.concatenate([np.arange(self.a_ptr[b], self.a_ptr[b + 1]) for b in ids])
            self._ids, self._ty = ids.copy(), torch.as_tensor(self.types[rows].astype(np.int32)).to(dev)
        g = build_batch_graph(self._ty, pos, self.cells[ids], self.pbcs[ids], self.cutoff, eng.spec.num_species,
                              n_atoms=self.n_atoms[ids], device=dev, species_rows=eng.needs_species_rows, cells_dev=cells_dev)
        out = eng.compute(g, want_atomic_virial=want_atomic_virial)
        self.n_force_calls += 1
        self.system_steps_evaluated += len(ids)
        fx = ex = self.virial_extra = None
        if self.extra is not None and with_extra:
            if getattr(self.extra, 'provides_virial', False):
                fx = self.extra(pos, g.seg_ptr_host, ids, cells_dev=cells_dev)
            else:
                fx = self.extra(pos, g.seg_ptr_host, ids)
            if isinstance(fx, tuple):
                if len(fx) == 3:
                    self.virial_extra = torch.as_tensor(fx[2]).to(dev, torch.float64).reshape(len(ids), 6).contiguous()
                fx, ex = fx[:2]
                ex = torch.as_tensor(ex).to(dev, torch.float64).reshape(len(ids))
            fx = torch.as_tensor(fx).to(dev, torch.float64).contiguous()
        return g, out, fx, ex


def batch_results(g: Graph, out: dict, cells, with_atomic_virial: bool = False) -> List[dict]:
    """one results dict per system of a batch graph `g` from the engine's output `out` for it: the keys, units, Voigt order
    and stress sign of SevenNetCalculator.compute (cells[B,3,3] gives the volumes)"""
    sp = g.seg_ptr_host
    e_sys = out['energy_per_system'].cpu().numpy()
    stress = virial_to_stress(out['virial_per_system'].cpu().numpy(), np.asarray(cells, np.float64).reshape(-1, 3, 3))
    energies = out['atomic_energy'].cpu().numpy().astype(np.float64)
    forces = out['forces'].cpu().numpy().astype(np.float64)
    n_edges = np.diff(g.row_ptr[torch.as_tensor(sp).to(g.row_ptr.device)].cpu().numpy())
    atomic_virial = out['atomic_virial'].cpu().numpy() if with_atomic_virial else None
    results = []
    for b in range(len(sp) - 1):
        a0, a1 = int(sp[b]), int(sp[b + 1])
        res = {'free_energy': float(e_sys[b]), 'energy': float(e_sys[b]), 'energies': energies[a0:a1],
               'forces': forces[a0:a1], 'stress': stress[b], 'num_edges': int(n_edges[b])}
        if atomic_virial is not None:
            res['stresses'] = atomic_virial[a0:a1]
        results.append(res)
    return results


def virial_to_stress(virial: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """[B,6] ASE Voigt stress (xx,yy,zz,yz,xz,xy, eV/A^3) from the engine's virial[B,6] (model order xx,yy,zz,xy,yz,zx) and
    cells[B,3,3]: -(virial / volume)[[0,1,2,4,5,3]] as SevenNetCalculator.compute (sevenn/calculator.py:198-203); NaN for a
    zero-volume cell"""
    virial = np.asarray(virial, np.float64).reshape(-1, 6)
    vol = np.abs(np.linalg.det(np.asarray(cells, np.float64).reshape(-1, 3, 3)))
    out = np.full(virial.shape, np.nan)
    ok = vol > 0
    out[ok] = -(virial[ok] / vol[ok, None])[:, [0, 1, 2, 4, 5, 3]]
    return out


def voigt_to_3x3(stress):
    """[..., 6] Voigt (xx,yy,zz,yz,xz,xy) -> [..., 3, 3] symmetric tensor (torch or numpy)"""
    idx = [[0, 5, 4], [5, 1, 3], [4, 3, 2]]
    if isinstance(stress, torch.Tensor):
        return stress[..., torch.as_tensor(idx, device=stress.device)]
    return np.asarray(stress)[..., np.asarray(idx)]
