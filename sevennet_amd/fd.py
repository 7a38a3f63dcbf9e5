"""Finite-difference copies: what vibrations (vib.py), supercell phonons (phonon.py) and elastic tensors (elastic.py) share.

Each of the three writes displaced or strained copies of its systems from base positions that were uploaded once, evaluates
them in batched force calls and reduces the results with kernels of its own.  Here are the plan of the copies (`plan_copies`),
the launch of the two kernels that write them (`write_copies`), the loop over the calls of a plan up to and including the force
call (`copy_calls`), the results of the unchanged copies in the keys of `compute_many` (`BaseCopies`) and the counters
(`call_info`).  The rows and finish launches, the one transfer and its unpacking stay with each driver.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Any, Callable, Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .batch import to_device, virial_to_stress

STENCIL = {2: (-1, 1), 4: (-2, -1, 1, 2)}   # the multipliers q of a row group, in the order of its copies


def check_extra(extra, make_extra) -> None:
    if extra is not None and make_extra is not None:
        raise ValueError('pass `extra` or `make_extra`, not both')


def plan_copies(n_atoms, selected: Optional[Sequence[np.ndarray]], nfree: int, max_atoms_per_call: int,
                n_groups: Optional[Sequence[int]] = None) -> SimpleNamespace:
    """The copies of B systems packed into calls (a pure function of its arguments).  n_atoms [B]; selected[b]: the displaced
    atoms of system b (indices within the system).  System b has 3 m_b ROW GROUPS -- the nfree copies of one (atom a, axis i), in
    the order of STENCIL[nfree] -- and one undisplaced copy.  Row groups are never split; a call holds at most
    `max_atoms_per_call` atoms unless it holds a single item (one row group, or one undisplaced copy: a system larger than the
    budget still runs); every (system, atom, axis, q) is planned exactly once.

    The force call sees COPY SLOTS as its systems: system b owns nfree g_b + 1 of them (g_b row groups and the undisplaced copy),
    with g_b = ceil(3 m_b / K) for the smallest number of calls K whose slots all fit the budget at once, so that slot counts are
    proportional to the systems' work, the systems finish together and all but the last calls use the same slots (a term planned
    per slot layout, d3.D3DeviceTerm, is then planned once and again where the layout thins out).  Where not even one row group
    per system fits, g_b = 1 and a call takes the systems that fit, in order.

    -> plan with `slot_system` int64 [S] (the system of each slot), `n_groups` [B] and `calls`: a list of namespaces with `ids`
    int64 [c] (the slots of the call's copies, ascending), `desc` int32 [c,4] (system, atom, axis, q per copy), `groups` int32
    [g,3] (first copy within the call, system, row r = 3 (position of a in selected[b]) + i) and `base` (pairs (copy within the
    call, system) of the undisplaced copies).

    n_groups [B]: the number of row groups of each system where they are not the coordinates of selected atoms (the six strain
    patterns of elastic.py).  `selected` is then not read, row r of system b is an index 0 .. n_groups[b] - 1 of the caller's, and
    the descriptor of its copies is (system, r, 0, q)."""
    n = np.asarray(n_atoms, np.int64).reshape(-1)
    B = len(n)
    qs = STENCIL[nfree]
    G = np.array([3 * len(s) for s in selected], np.int64) if n_groups is None else np.array(n_groups, np.int64).reshape(-1)
    budget = int(max_atoms_per_call)
    g = np.ones(B, np.int64)
    lo, hi = 1, int(G.max())   # the smallest K whose slots fit (the slots' atom count does not grow with K)
    fits = lambda K: int((n * (nfree * -(-G // K) + 1)).sum()) <= budget   # noqa: E731
    if fits(hi):
        while lo < hi:
            mid = (lo + hi) // 2
            if fits(mid):
                hi = mid
            else:
                lo = mid + 1
        g = -(-G // lo)
    slot0 = np.concatenate([[0], np.cumsum(nfree * g + 1)])
    slot_system = np.repeat(np.arange(B), nfree * g + 1)
    pending, next_row, base_done = G.copy(), np.zeros(B, np.int64), np.zeros(B, bool)
    calls = []
    while (pending > 0).any() or not base_done.all():
        ids, desc, groups, base = [], [], [], []
        used = n_items = 0
        for b in range(B):
            if pending[b] > 0:
                t = int(min(g[b], pending[b], (budget - used) // (nfree * n[b])))
                if t <= 0 and n_items == 0:
                    t = 1
                for k in range(max(t, 0)):
                    r = int(next_row[b]) + k
                    groups.append((len(desc), b, r))
                    for w, q in enumerate(qs):
                        ids.append(slot0[b] + nfree * k + w)
                        desc.append((b, int(selected[b][r // 3]), r % 3, q) if n_groups is None else (b, r, 0, q))
                if t > 0:
                    used += t * nfree * int(n[b])
                    n_items += t
                    pending[b] -= t
                    next_row[b] += t
            if pending[b] == 0 and not base_done[b] and (used + n[b] <= budget or n_items == 0):
                base.append((len(desc), b))
                ids.append(slot0[b] + nfree * g[b])
                desc.append((b, 0, 0, 0))
                used += int(n[b])
                n_items += 1
                base_done[b] = True
        calls.append(SimpleNamespace(ids=np.asarray(ids, np.int64), desc=np.asarray(desc, np.int32).reshape(-1, 4),
                                     groups=np.asarray(groups, np.int32).reshape(-1, 3), base=base, n_atoms=used))
    return SimpleNamespace(slot_system=slot_system, n_groups=G, calls=calls, nfree=nfree)


def write_copies(symbol: str, width: int, pos0: torch.Tensor, seg_ptr0: torch.Tensor, desc: torch.Tensor, copy_ptr: torch.Tensor,
                 delta: float, pos_out: torch.Tensor, status: torch.Tensor) -> None:
    """one launch of a kernel that writes copies, on the current stream: `snet_vib_displace` (desc [c,4]) or `snet_el_strain` (desc
    [c,3]), which have one argument list (dtypes as the C ABI: pos0 / pos_out fp64, the rest int32)"""
    n0, n_sys, n_copies, n_out = int(pos0.shape[0]), int(seg_ptr0.numel()) - 1, int(desc.shape[0]), int(pos_out.shape[0])
    f64, i32 = torch.float64, torch.int32
    _lib.check_device_tensors(symbol[len('snet_'):], pos0, [(pos0, f64, (n0, 3)), (seg_ptr0, i32, (n_sys + 1,)),
                                                            (desc, i32, (n_copies, width)), (copy_ptr, i32, (n_copies + 1,)),
                                                            (pos_out, f64, (n_out, 3)), (status, i32, (n_copies,))])
    P = _lib.ptr
    with torch.cuda.device(pos0.device):
        _lib.check(getattr(_lib.load(), symbol)(P(pos0), n0, P(seg_ptr0), n_sys, P(desc), P(copy_ptr), n_copies, float(delta),
                                                P(pos_out), n_out, P(status), _lib.stream()), symbol)


def copy_calls(forces, calls, pos0: torch.Tensor, seg_ptr0: torch.Tensor, n_atoms: np.ndarray, writer: Callable, delta: float,
               refused: List[torch.Tensor], want_atomic_virial: bool = False, keeper: Optional[Callable] = None) -> Iterator:
    """The calls of a plan up to the reduction: per call one launch of `writer` (vib.vib_displace, elastic.el_strain) that writes
    the call's copies from the base positions pos0 (fp64 [sum n_b, 3], seg_ptr0 int32 [B+1], both on the device; n_atoms [B] on
    the host), one force call and, if given, keeper(call, graph, output, extra forces) (`BaseCopies`); then (call, graph, output,
    extra forces) is handed to the caller for its rows launch.  Nothing is read back: the status of each call's copies is appended
    to `refused`, for `refused_count`.  forces: a BatchForces over the slots of the plan, or any object with its call interface;
    want_atomic_virial asks the calls that hold an unchanged copy for the per-atom virial."""
    dev, f64, i32 = pos0.device, torch.float64, torch.int32
    for call in calls:
        copy_ptr = np.concatenate([[0], np.cumsum(n_atoms[call.desc[:, 0]])])
        pos = torch.empty(int(copy_ptr[-1]), 3, dtype=f64, device=dev)
        st = torch.zeros(len(call.ids), dtype=i32, device=dev)
        writer(pos0, seg_ptr0, to_device(call.desc, i32, dev), to_device(copy_ptr, i32, dev), delta, pos, st)
        refused.append(st)
        g, out, fx, _ = forces(pos, call.ids, want_atomic_virial=want_atomic_virial and bool(call.base))
        if keeper is not None:
            keeper(call, g, out, fx)
        yield call, g, out, fx


def refused_count(refused: List[torch.Tensor]) -> torch.Tensor:
    """fp64 [1] on the device: how many copies the writer refused, for the driver's one transfer"""
    return torch.cat(refused).sum().to(torch.float64).reshape(1)


def check_refused(count, writer: Callable) -> None:
    if count != 0:
        raise RuntimeError(f'snet_{writer.__name__} refused {int(count)} copies of the plan: its descriptors do not fit the systems')


def call_info(forces, calls, n_other_launches: int) -> Dict[str, int]:
    """the counters of a driver: per call one writer launch and, where it holds row groups, one rows launch, plus the caller's"""
    return dict(n_force_calls=forces.n_force_calls, copies_evaluated=int(sum(len(c.ids) for c in calls)),
                launches=len(calls) + sum(1 for c in calls if len(c.groups)) + n_other_launches)


class BaseCopies:
    """The results of the unchanged copies (`call.base`), kept on the device while the calls run: the keeper of `copy_calls`.
    keep_extra: also the rows of the extra forces, where there are any."""

    def __init__(self, want_atomic_virial: bool = False, keep_extra: bool = False):
        self.want_atomic_virial, self.keep_extra = want_atomic_virial, keep_extra
        self.kept = []   # per call with unchanged copies: (systems, device tensors of their results)

    def __call__(self, call, g, out, fx=None) -> None:
        if not call.base:
            return
        dev = out['forces'].device
        sp = g.seg_ptr_host
        copies = np.array([j for j, _ in call.base], np.int64)
        rows = torch.as_tensor(np.concatenate([np.arange(sp[j], sp[j + 1]) for j in copies])).to(dev)
        j_d = torch.as_tensor(copies).to(dev)
        rp = g.row_ptr.long()
        took = dict(energy=out['energy_per_system'][j_d].clone(), virial=out['virial_per_system'][j_d].clone(),
                    forces=out['forces'][rows].clone(), energies=out['atomic_energy'][rows].clone(),
                    n_edges=rp[torch.as_tensor(sp[copies + 1]).to(dev)] - rp[torch.as_tensor(sp[copies]).to(dev)])
        if self.keep_extra and fx is not None:
            took['forces_extra'] = fx[rows].clone()
        if self.want_atomic_virial:
            took['stresses'] = out['atomic_virial'][rows].clone()
        self.kept.append(([b for _, b in call.base], took))

    def results(self, n_atoms, cells, energies_key: str = 'energies') -> List[Dict[str, Any]]:
        """One dict per system, in system order, with the keys of batch.batch_results (the per-atom energies under
        `energies_key`) and, where they were kept, `forces_extra` fp64 [n_b,3].  n_atoms [B] and cells [B,3,3] of the copies;
        one transfer per kept tensor."""
        results: List[Optional[Dict[str, Any]]] = [None] * len(n_atoms)
        for systems, took in self.kept:
            host = {k: v.cpu().numpy() for k, v in took.items()}
            stress = virial_to_stress(host['virial'], cells[systems])
            r0 = 0
            for k, b in enumerate(systems):
                r1 = r0 + int(n_atoms[b])
                res = {'free_energy': float(host['energy'][k]), 'energy': float(host['energy'][k]),
                       energies_key: host['energies'][r0:r1].astype(np.float64), 'forces': host['forces'][r0:r1].astype(np.float64),
                       'stress': stress[k], 'num_edges': int(host['n_edges'][k])}
                for key in ('stresses', 'forces_extra'):
                    if key in host:
                        res[key] = host[key][r0:r1]
                results[b] = res
                r0 = r1
        return results
