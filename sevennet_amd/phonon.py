"""Batched supercell phonons: force constants of the home-cell atoms against the whole supercell by finite displacements, the
nearest-image rule and the dynamical matrices D(q) of many q-points, for many crystals at once.

The rule is written out in include/snet_hip.h ("batched supercell phonons") and restated in fp64 numpy in tests/phonon_ref.py.
System b is a primitive cell with m_b atoms and repeats (n1,n2,n3); `build_supercell` makes its N_b = m_b n1 n2 n3 atoms on the host,
once, home cell first.  Only the m_b home atoms are displaced: `fd.plan_copies` packs the nfree 3 m_b displaced supercells and the
undisplaced one of every system into calls of at most `max_atoms_per_call` atoms, and per call `snet_vib_displace` writes the copies,
one batched evaluation (sevennet_amd.batch) gives their forces and `snet_ph_rows` writes the rows of Phi [3 m_b, 3 N_b] they
determine (written once each, so the result does not depend on the packing).  After the calls `snet_ph_finish` measures and, if
asked, enforces the acoustic sum rule, `snet_ph_images` finds the nearest images of every (home atom, supercell atom) pair, and
`snet_ph_dynmat` assembles D(q) for the path and mesh points of all systems, at most `max_q_per_call` q-points per launch.  One
transfer brings Phi, D(q) and the counters to the host, where numpy.linalg.eigh, the density of states and the harmonic
thermodynamics run: the matrices are tiny against the force calls.

The phase of D(q) is taken with the full vector between the two atoms, exp(i q . (r_j - r_alpha + n S)), so the eigenvectors
(`modes`) are in that convention: they carry no further factor exp(i q . r_beta).
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .batch import BatchForces, _as_host, device_positions, to_device, validate_batch_inputs
from .fd import BaseCopies, call_info, check_extra, check_refused, copy_calls, plan_copies, refused_count
from .md import ACC, KB
from .vib import HBAR, INV_CM, VIB_STATUS_NAMES, validate_vib_inputs, vib_displace

REDUCED_SLACK = 1e-9   # |s_i|^2 <= |s_i + x s_j + y s_k|^2 (1 + this)


# ------------------------------------------------------------------------------------------------ host: cells, q-points
def is_reduced(S) -> bool:
    """the condition under which the 27 candidates n0 + {-1,0,1}^3 hold every nearest image: no row of S [3,3] gets shorter by adding
    -1, 0 or 1 times each of the other two"""
    S = np.asarray(S, np.float64).reshape(3, 3)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        own = S[i] @ S[i]
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                v = S[i] + x * S[j] + y * S[k]
                if not own <= (v @ v) * (1.0 + REDUCED_SLACK):
                    return False
    return True


def validate_phonon_inputs(n_atoms, cells, pbcs, supercells, qpoints=None, mesh=None, temperatures=None, symprec=1e-5, e_min=1e-5,
                           dos_bins=200, max_q_per_call=4096):
    """The arguments of `phonons_batch` that `validate_batch_inputs` and `vib.validate_vib_inputs` do not see, on the host
    (ValueError names the system).  n_atoms [B], cells [B,3,3], pbcs [B,3] as validate_batch_inputs returns them; supercells: one
    triple of repeats for all systems or one per system; qpoints: None, one [n_q,3] array of fractional q-points for all systems or
    a list of one per system; mesh: None or a triple of integers >= 1; temperatures: None or kelvins >= 0.
    -> (repeats int64 [B,3], q-points per system fp64 [n_q,3] (n_q may be 0 with a mesh), mesh tuple or None, temperatures fp64)"""
    n_atoms = np.asarray(n_atoms, np.int64).reshape(-1)
    B = len(n_atoms)
    cells = np.asarray(cells, np.float64).reshape(B, 3, 3)
    pbcs = np.asarray(pbcs, bool).reshape(B, 3)

    def triple(x, what):
        a = np.asarray(x)
        if a.shape != (3,) or a.dtype == bool or not np.issubdtype(a.dtype, np.integer) or (a < 1).any():
            raise ValueError(f'{what} = {x!r}: three integers >= 1 are required')
        return a.astype(np.int64)

    reps = np.asarray(supercells)
    if reps.ndim == 1:
        repeats = np.tile(triple(supercells, 'supercells'), (B, 1))
    elif reps.ndim == 2 and len(reps) == B:
        repeats = np.stack([triple(supercells[b], f'system {b}: supercell') for b in range(B)])
    else:
        raise ValueError(f'supercells: one triple of repeats, or one per system ({B}), is required')
    for b in range(B):
        if n_atoms[b] < 1:
            raise ValueError(f'system {b}: a crystal has at least one atom')
        if not pbcs[b].all():
            raise ValueError(f'system {b}: phonons need a fully periodic system, got pbc = {pbcs[b].tolist()}')
        if not np.isfinite(cells[b]).all() or abs(np.linalg.det(cells[b])) <= 0.0:
            raise ValueError(f'system {b}: the cell is singular or not finite')
        if not is_reduced(repeats[b][:, None] * cells[b]):
            raise ValueError(f'system {b}: the supercell diag({repeats[b].tolist()}) C is not reduced (a lattice vector gets shorter by '
                             'adding others), so the nearest images are not among the 27 candidates: pass a reduced cell '
                             '(Niggli or Minkowski) or other repeats')
    if qpoints is None and mesh is None:
        raise ValueError('pass `qpoints`, `mesh` or both: there is nothing to compute otherwise')
    if qpoints is None:
        q_list = [np.zeros((0, 3))] * B
    else:
        if isinstance(qpoints, (list, tuple)) and len(qpoints) == B and all(np.ndim(q) == 2 for q in qpoints):
            q_list = [np.asarray(q, np.float64) for q in qpoints]
        elif np.ndim(qpoints) == 2:
            q_list = [np.asarray(qpoints, np.float64)] * B
        else:
            raise ValueError(f'qpoints: None, one [n_q,3] array or one per system ({B}) is required')
        for b, q in enumerate(q_list):
            if q.ndim != 2 or q.shape[1] != 3 or not np.isfinite(q).all():
                raise ValueError(f'system {b}: q-points are a finite [n_q,3] array of fractional coordinates, got shape {q.shape}')
            if len(q) == 0 and mesh is None:
                raise ValueError(f'system {b}: no q-point is given')
    if mesh is not None:
        mesh = tuple(int(x) for x in triple(mesh, 'mesh'))
    if temperatures is None:
        temps = np.zeros(0)
    else:
        if mesh is None:
            raise ValueError('temperatures need a `mesh` to sum over')
        temps = np.atleast_1d(np.asarray(temperatures, np.float64))
        if temps.ndim != 1 or not (np.isfinite(temps) & (temps >= 0)).all():
            raise ValueError(f'temperatures = {temperatures!r}: finite temperatures >= 0 in K are required')
    for name, val in (('symprec', symprec), ('e_min', e_min)):
        try:
            ok = bool(np.isfinite(val)) and val >= 0 and not isinstance(val, bool)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f'{name} = {val!r}: a finite number >= 0 is required')
    if isinstance(dos_bins, (int, np.integer)) and not isinstance(dos_bins, bool):
        if dos_bins < 1:
            raise ValueError(f'dos_bins = {dos_bins!r}: a count >= 1 or increasing bin edges are required')
    else:
        try:
            edges = np.asarray(dos_bins, np.float64)
        except (TypeError, ValueError):
            edges = np.zeros(0)
        if isinstance(dos_bins, bool) or edges.ndim != 1 or len(edges) < 2 or not np.isfinite(edges).all() or (np.diff(edges) <= 0).any():
            raise ValueError(f'dos_bins = {dos_bins!r}: a count >= 1 or increasing bin edges are required')
    if isinstance(max_q_per_call, bool) or not isinstance(max_q_per_call, (int, np.integer)) or max_q_per_call < 1:
        raise ValueError(f'max_q_per_call = {max_q_per_call!r}: an integer >= 1 is required')
    return repeats, q_list, mesh, temps


def build_supercell(types, positions, cell, repeats) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (types [N], positions [N,3], S [3,3]) of the supercell diag(repeats) cell: atom c m + beta is atom beta shifted by
    (c1,c2,c3) cell with c = (c1 n2 + c2) n3 + c3, so the home cell comes first"""
    types, positions = np.asarray(types).reshape(-1), np.asarray(positions, np.float64).reshape(-1, 3)
    cell, n = np.asarray(cell, np.float64).reshape(3, 3), np.asarray(repeats, np.int64).reshape(3)
    c = np.stack(np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    shift = c @ cell
    return np.tile(types, len(c)), (shift[:, None, :] + positions[None, :, :]).reshape(-1, 3), n[:, None].astype(np.float64) * cell


def band_path(points, n_per_segment: int) -> np.ndarray:
    """fractional q-points along the straight segments between `points` [P,3]: n_per_segment steps per segment, the end of one
    segment being the start of the next (listed once) -> [(P - 1) n_per_segment + 1, 3]"""
    pts = np.asarray(points, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or len(pts) < 2 or not np.isfinite(pts).all():
        raise ValueError(f'band_path: at least two finite points [P,3] are required, got shape {pts.shape}')
    if isinstance(n_per_segment, bool) or not isinstance(n_per_segment, (int, np.integer)) or n_per_segment < 1:
        raise ValueError(f'band_path: n_per_segment = {n_per_segment!r}: an integer >= 1 is required')
    t = np.arange(n_per_segment, dtype=np.float64)[:, None] / n_per_segment
    out = [pts[s] + t * (pts[s + 1] - pts[s]) for s in range(len(pts) - 1)]
    return np.concatenate(out + [pts[-1:]])


def mesh_points(mesh) -> np.ndarray:
    """the Gamma-centred mesh (i/n1, j/n2, k/n3), every point with the same weight, no symmetry reduction -> [n1 n2 n3, 3]"""
    n = np.asarray(mesh, np.int64).reshape(3)
    g = np.stack(np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing='ij'), -1).reshape(-1, 3)
    return g / n.astype(np.float64)


# ------------------------------------------------------------------------------------------------ host: spectrum, sums
def spectrum(D: np.ndarray, want_modes: bool = False) -> Dict[str, Any]:
    """eigenvalues [n_q,3m] (ascending, eV/(A^2 amu)), signed energies h nu (eV) and frequencies (cm^-1) -- an imaginary mode is a
    negative number -- of stacked Hermitian matrices D [n_q,3m,3m], as vib.spectrum; with want_modes also `modes` [n_q,3m,m,3]
    complex (row k belongs to eigenvalues[k]).  NaN throughout where D is not finite."""
    n_q, k = D.shape[0], D.shape[1]
    if n_q == 0 or not np.isfinite(D).all():
        lam = np.full((n_q, k), np.nan)
        vec = np.full((n_q, k, k), np.nan, np.complex128)
    else:
        lam, vec = np.linalg.eigh(D)
    e = HBAR * np.sqrt(ACC * np.abs(lam)) * np.sign(lam)
    out = dict(eigenvalues=lam, energies=e, frequencies=e * INV_CM)
    if want_modes:
        out['modes'] = np.ascontiguousarray(np.swapaxes(vec, 1, 2)).reshape(n_q, k, k // 3, 3)
    return out


def thermodynamics(energies, temperatures, e_min: float = 1e-5) -> Dict[str, Any]:
    """Harmonic free energy, entropy and heat capacity per primitive cell from the signed mode energies h nu (eV) of an equal-weight
    mesh, `energies` [n_mesh, 3m].  Over the modes with h nu > e_min, averaged over the mesh, with x = h nu / kT:
    F = sum [h nu / 2 + kT ln(1 - e^-x)], S = k_B sum [x / (e^x - 1) - ln(1 - e^-x)], C_v = k_B sum x^2 e^x / (e^x - 1)^2; at T = 0
    F = zpe and S = C_v = 0.  -> dict(temperatures [K], free_energy [eV], entropy and heat_capacity [eV/K], zpe [eV], n_imaginary
    (modes with h nu < -e_min, left out of the sums) and n_skipped (|h nu| <= e_min)); NaN where the energies are not finite."""
    e = np.asarray(energies, np.float64)
    e = e.reshape(-1, e.shape[-1]) if e.ndim >= 2 else e.reshape(1, -1)
    T = np.atleast_1d(np.asarray(temperatures, np.float64))
    n_mesh = e.shape[0]
    if not np.isfinite(e).all():
        nan = np.full(len(T), np.nan)
        return dict(temperatures=T.copy(), free_energy=nan, entropy=nan.copy(), heat_capacity=nan.copy(), zpe=float('nan'),
                    n_imaginary=0, n_skipped=0)
    flat = e.reshape(-1)
    hv = flat[flat > e_min]
    zpe = float(0.5 * hv.sum() / n_mesh)
    F, S, Cv = np.zeros(len(T)), np.zeros(len(T)), np.zeros(len(T))
    for t, temp in enumerate(T):
        if temp == 0.0:
            F[t] = zpe
            continue
        kT = KB * temp
        x = hv / kT
        log_term = np.log1p(-np.exp(-x))       # ln(1 - e^-x)
        F[t] = (0.5 * hv + kT * log_term).sum() / n_mesh
        decay = np.exp(-x)                     # (x / (e^x - 1) = x e^-x / (1 - e^-x): nothing overflows at large x)
        S[t] = KB * (x * decay / -np.expm1(-x) - log_term).sum() / n_mesh
        Cv[t] = KB * (x * x * decay / np.expm1(-x) ** 2).sum() / n_mesh   # x^2 e^x / (e^x - 1)^2
    return dict(temperatures=T.copy(), free_energy=F, entropy=S, heat_capacity=Cv, zpe=zpe, n_imaginary=int((flat < -e_min).sum()),
                n_skipped=int((np.abs(flat) <= e_min).sum()))


def dos(energies, dos_bins=200) -> Tuple[np.ndarray, np.ndarray]:
    """The density of states of an equal-weight mesh: numpy.histogram of the signed mode energies [n_mesh, 3m] over dos_bins (a
    count or explicit edges), divided by n_mesh and the bin widths, so that it integrates to 3m when the bins hold every mode.
    -> (bin centres [eV], states per eV and primitive cell); NaN where the energies are not finite."""
    e = np.asarray(energies, np.float64)
    e = e.reshape(-1, e.shape[-1])
    if not np.isfinite(e).all():
        n = dos_bins if isinstance(dos_bins, (int, np.integer)) else len(dos_bins) - 1
        return np.full(n, np.nan), np.full(n, np.nan)
    hist, edges = np.histogram(e.reshape(-1), bins=dos_bins)
    return 0.5 * (edges[1:] + edges[:-1]), hist / (e.shape[0] * np.diff(edges))


# ------------------------------------------------------------------------------------------------ launches
def ph_rows(forces: torch.Tensor, forces_extra: Optional[torch.Tensor], seg_ptr: torch.Tensor, group: torch.Tensor, nfree: int,
            delta: float, m_ptr: torch.Tensor, sc_ptr: torch.Tensor, p_off: torch.Tensor, phi: torch.Tensor, status: torch.Tensor) -> None:
    """one `snet_ph_rows` launch on the current stream (forces fp32, forces_extra / phi fp64, p_off int64, the rest int32)"""
    N, n_copies, n_groups = int(forces.shape[0]), int(seg_ptr.numel()) - 1, int(group.shape[0])
    n_sys, p_size = int(m_ptr.numel()) - 1, int(phi.numel())
    f64, i32 = torch.float64, torch.int32
    want = [(forces, torch.float32, (N, 3)), (seg_ptr, i32, (n_copies + 1,)), (group, i32, (n_groups, 3)), (m_ptr, i32, (n_sys + 1,)),
            (sc_ptr, i32, (n_sys + 1,)), (p_off, torch.int64, (n_sys,)), (phi, f64, (p_size,)), (status, i32, (n_sys,))]
    if forces_extra is not None:
        want.append((forces_extra, f64, (N, 3)))
    _lib.check_device_tensors('ph_rows', phi, want)
    P = _lib.ptr
    with torch.cuda.device(phi.device):
        _lib.check(_lib.load().snet_ph_rows(P(forces), P(forces_extra), N, P(seg_ptr), n_copies, P(group), n_groups, int(nfree),
                                            float(delta), P(m_ptr), P(sc_ptr), P(p_off), n_sys, P(phi), p_size, P(status),
                                            _lib.stream()), 'snet_ph_rows')


def ph_finish(phi: torch.Tensor, p_off: torch.Tensor, m_ptr: torch.Tensor, sc_ptr: torch.Tensor, acoustic: bool, status: torch.Tensor,
              phi_out: torch.Tensor, asr_defect: torch.Tensor) -> None:
    """one `snet_ph_finish` launch on the current stream (phi / phi_out / asr_defect fp64, p_off int64, the rest int32)"""
    n_sys, p_size = int(m_ptr.numel()) - 1, int(phi.numel())
    f64, i32 = torch.float64, torch.int32
    _lib.check_device_tensors('ph_finish', phi, [(phi, f64, (p_size,)), (p_off, torch.int64, (n_sys,)), (m_ptr, i32, (n_sys + 1,)),
                                                 (sc_ptr, i32, (n_sys + 1,)), (status, i32, (n_sys,)), (phi_out, f64, (p_size,)),
                                                 (asr_defect, f64, (n_sys,))])
    P = _lib.ptr
    with torch.cuda.device(phi.device):
        _lib.check(_lib.load().snet_ph_finish(P(phi), P(p_off), P(m_ptr), P(sc_ptr), n_sys, p_size, int(bool(acoustic)), P(status),
                                              P(phi_out), P(asr_defect), _lib.stream()), 'snet_ph_finish')


def ph_images(pos: torch.Tensor, sc_ptr: torch.Tensor, m_ptr: torch.Tensor, home_sys: torch.Tensor, S: torch.Tensor, S_inv: torch.Tensor,
              i_off: torch.Tensor, symprec: float, img_base: torch.Tensor, img_mask: torch.Tensor, status: torch.Tensor) -> None:
    """one `snet_ph_images` launch on the current stream (pos / S / S_inv fp64, i_off int64, the rest int32)"""
    n_atoms, n_sys, n_home, i_size = int(pos.shape[0]), int(m_ptr.numel()) - 1, int(home_sys.numel()), int(img_mask.numel())
    f64, i32 = torch.float64, torch.int32
    _lib.check_device_tensors('ph_images', pos, [(pos, f64, (n_atoms, 3)), (sc_ptr, i32, (n_sys + 1,)), (m_ptr, i32, (n_sys + 1,)),
                                                 (home_sys, i32, (n_home,)), (S, f64, (n_sys, 9)), (S_inv, f64, (n_sys, 9)),
                                                 (i_off, torch.int64, (n_sys,)), (img_base, i32, (i_size, 3)), (img_mask, i32, (i_size,)),
                                                 (status, i32, (n_sys,))])
    P = _lib.ptr
    with torch.cuda.device(pos.device):
        _lib.check(_lib.load().snet_ph_images(P(pos), n_atoms, P(sc_ptr), P(m_ptr), P(home_sys), n_home, P(S), P(S_inv), P(i_off), n_sys,
                                              float(symprec), P(img_base), P(img_mask), i_size, P(status), _lib.stream()), 'snet_ph_images')


def ph_dynmat(phi: torch.Tensor, p_off: torch.Tensor, pos: torch.Tensor, sc_ptr: torch.Tensor, m_ptr: torch.Tensor, w: torch.Tensor,
              S: torch.Tensor, img_base: torch.Tensor, img_mask: torch.Tensor, i_off: torch.Tensor, q_cart: torch.Tensor,
              q_sys: torch.Tensor, q_ptr: torch.Tensor, d_off: torch.Tensor, max_m: int, status: torch.Tensor, R: torch.Tensor,
              D: torch.Tensor, hermiticity: torch.Tensor) -> None:
    """one `snet_ph_dynmat` call (two launches) on the current stream (phi / pos / w / S / q_cart / R / D / hermiticity fp64, p_off /
    i_off / d_off int64, the rest int32; R and D [d_size,2]: real and imaginary parts)"""
    n_atoms, n_sys, n_home, i_size = int(pos.shape[0]), int(m_ptr.numel()) - 1, int(w.numel()), int(img_mask.numel())
    p_size, n_q, d_size = int(phi.numel()), int(q_sys.numel()), int(R.shape[0])
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    _lib.check_device_tensors('ph_dynmat', phi, [(phi, f64, (p_size,)), (p_off, i64, (n_sys,)), (pos, f64, (n_atoms, 3)),
                                                 (sc_ptr, i32, (n_sys + 1,)), (m_ptr, i32, (n_sys + 1,)), (w, f64, (n_home,)),
                                                 (S, f64, (n_sys, 9)), (img_base, i32, (i_size, 3)), (img_mask, i32, (i_size,)),
                                                 (i_off, i64, (n_sys,)), (q_cart, f64, (n_q, 3)), (q_sys, i32, (n_q,)),
                                                 (q_ptr, i32, (n_sys + 1,)), (d_off, i64, (n_sys,)), (status, i32, (n_sys,)),
                                                 (R, f64, (d_size, 2)), (D, f64, (d_size, 2)), (hermiticity, f64, (n_q,))])
    P = _lib.ptr
    with torch.cuda.device(phi.device):
        _lib.check(_lib.load().snet_ph_dynmat(P(phi), P(p_off), p_size, P(pos), n_atoms, P(sc_ptr), P(m_ptr), P(w), n_home, P(S),
                                              P(img_base), P(img_mask), P(i_off), i_size, P(q_cart), P(q_sys), P(q_ptr), n_q, P(d_off),
                                              n_sys, int(max_m), P(status), P(R), P(D), d_size, P(hermiticity), _lib.stream()),
                   'snet_ph_dynmat')


# ------------------------------------------------------------------------------------------------ the loop
def phonon_loop(forces, plan, positions, n_super, n_home, masses, supercell_cells, q_cart: Sequence[np.ndarray], *, delta: float,
                acoustic: bool = True, symprec: float = 1e-5, max_q_per_call: int = 4096, keeper: Optional[Callable] = None,
                want_atomic_virial: bool = False):
    """The calls of a plan, then the sum rule, the images and D(q).  forces: a BatchForces over the copy slots of `plan` (made by
    fd.plan_copies with n_atoms = n_super and the home atoms selected), or any object with its call interface; positions: the flat
    supercell positions [sum N_b, 3], home cell first; n_super / n_home [B]; masses: per system, of the home atoms (amu);
    supercell_cells [B,3,3]; q_cart[b] [n_q_b, 3] in rad/A (n_q_b >= 1).  Per call one `snet_vib_displace`, one force call and one
    `snet_ph_rows`, nothing read back; keeper as in vib.vib_loop.  Then one `snet_ph_finish`, one `snet_ph_images`, one
    `snet_ph_dynmat` per at most `max_q_per_call` q-points (its R is dropped after each: the cap bounds that buffer, 144 m^2 bytes per
    q-point) and one transfer.
    -> (force constants: per system [m,N,3,3]; asr_defect [B]; D: per system complex [n_q,3m,3m]; hermiticity: per system [n_q];
    status [B] (0 ok, 2 a non-finite force, 3 a layout the kernels refused); info)"""
    dev = forces.engine.dev
    N, m = np.asarray(n_super, np.int64).reshape(-1), np.asarray(n_home, np.int64).reshape(-1)
    B, nfree = len(N), plan.nfree
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    p_off = np.concatenate([[0], np.cumsum(9 * m * N)])
    i_off = np.concatenate([[0], np.cumsum(m * N)])
    n_q = np.array([len(q) for q in q_cart], np.int64)
    q_start = np.concatenate([[0], np.cumsum(n_q)])
    q_sys = np.repeat(np.arange(B), n_q)
    S = np.asarray(supercell_cells, np.float64).reshape(B, 3, 3)
    with torch.cuda.device(dev):
        pos0 = device_positions(positions, dev).contiguous()
        sc_ptr, m_ptr = (to_device(np.concatenate([[0], np.cumsum(k)]), i32, dev) for k in (N, m))
        off_d = to_device(p_off[:-1], i64, dev)
        phi = torch.zeros(int(p_off[-1]), dtype=f64, device=dev)
        status = torch.zeros(B, dtype=i32, device=dev)
        refused = []
        for call, g, out, fx in copy_calls(forces, plan.calls, pos0, sc_ptr, N, vib_displace, delta, refused, want_atomic_virial, keeper):
            if len(call.groups):
                ph_rows(out['forces'], fx, g.seg_ptr, to_device(call.groups, i32, dev), nfree, delta, m_ptr, sc_ptr, off_d, phi, status)
        phi_out, asr = torch.empty_like(phi), torch.empty(B, dtype=f64, device=dev)
        ph_finish(phi, off_d, m_ptr, sc_ptr, acoustic, status, phi_out, asr)
        S_d, Si_d = to_device(S.reshape(B, 9), f64, dev), to_device(np.linalg.inv(S).reshape(B, 9), f64, dev)
        ioff_d = to_device(i_off[:-1], i64, dev)
        img_base = torch.empty(int(i_off[-1]), 3, dtype=i32, device=dev)
        img_mask = torch.empty(int(i_off[-1]), dtype=i32, device=dev)
        ph_images(pos0, sc_ptr, m_ptr, to_device(np.repeat(np.arange(B), m), i32, dev), S_d, Si_d, ioff_d, symprec, img_base, img_mask,
                  status)
        w_d = to_device(np.concatenate([1.0 / np.sqrt(np.asarray(ms, np.float64)) for ms in masses]), f64, dev)
        q_all = to_device(np.concatenate([np.asarray(q, np.float64).reshape(-1, 3) for q in q_cart]), f64, dev)
        D_parts, herm_parts, n_dyn = [], [], 0
        for g0 in range(0, int(q_start[-1]), int(max_q_per_call)):
            g1 = min(g0 + int(max_q_per_call), int(q_start[-1]))
            q_ptr = np.clip(q_start, g0, g1) - g0
            d_off = np.concatenate([[0], np.cumsum(np.diff(q_ptr) * 9 * m * m)])
            R = torch.empty(int(d_off[-1]), 2, dtype=f64, device=dev)
            D, herm = torch.empty_like(R), torch.empty(g1 - g0, dtype=f64, device=dev)
            ph_dynmat(phi_out, off_d, pos0, sc_ptr, m_ptr, w_d, S_d, img_base, img_mask, ioff_d, q_all[g0:g1].contiguous(),
                      to_device(q_sys[g0:g1], i32, dev), to_device(q_ptr, i32, dev), to_device(d_off[:-1], i64, dev), int(m.max()), status,
                      R, D, herm)
            D_parts.append(D.reshape(-1))
            herm_parts.append(herm)
            n_dyn += 1
        flat = torch.cat([phi_out, asr] + D_parts + herm_parts + [status.to(f64), refused_count(refused)]).cpu().numpy()   # the one transfer
    check_refused(flat[-1], vib_displace)
    size, n_qt = int(p_off[-1]), int(q_start[-1])
    phi_h = [flat[p_off[b]:p_off[b + 1]].reshape(m[b], 3, N[b], 3).transpose(0, 2, 1, 3).copy() for b in range(B)]
    asr_h = flat[size:size + B].copy()
    d_ptr = size + B + 2 * np.concatenate([[0], np.cumsum(n_q * 9 * m * m)])   # (the chunks follow the order of the q-points)
    D_h = []
    for b in range(B):
        blk = flat[d_ptr[b]:d_ptr[b + 1]].reshape(n_q[b], 3 * m[b], 3 * m[b], 2)
        D_h.append(blk[..., 0] + 1j * blk[..., 1])
    h0 = int(d_ptr[-1])
    herm_h = [flat[h0 + q_start[b]:h0 + q_start[b + 1]].copy() for b in range(B)]
    status_h = flat[h0 + n_qt:h0 + n_qt + B].astype(np.int64)
    return phi_h, asr_h, D_h, herm_h, status_h, dict(call_info(forces, plan.calls, 2 + n_dyn), q_evaluated=n_qt)


# ------------------------------------------------------------------------------------------------ the driver
def phonons_batch(engine, types, positions, masses, cells, pbcs, supercells, *, cutoff: float, qpoints=None, mesh=None,
                  temperatures=None, delta: float = 0.01, nfree: int = 2, acoustic: bool = True, symprec: float = 1e-5,
                  want_modes: bool = False, dos_bins=200, e_min: float = 1e-5, max_atoms_per_call: int = 32768,
                  max_q_per_call: int = 4096, extra: Optional[Callable] = None, make_extra: Optional[Callable] = None, n_atoms=None,
                  want_atomic_virial: bool = False) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """Supercell phonons of B crystals at once.

    engine: a HipForceEngine; types / positions / cells / pbcs / n_atoms describe the PRIMITIVE cells as batch.build_batch_graph
    takes them (pbc all true); masses in amu, per system or flat; supercells: the repeats (n1,n2,n3), one triple or one per system.
    qpoints: fractional q-points of the primitive reciprocal lattice ([n_q,3] for all systems or one array per system; `band_path`
    makes a path); mesh: (n1',n2',n3') of a Gamma-centred mesh for the density of states and, with temperatures (K), the harmonic
    thermodynamics; at least one of the two.  delta / nfree / max_atoms_per_call as vib.vibrations_batch; acoustic: enforce the
    acoustic sum rule on the self terms; symprec (A): images within it of the nearest share the weight; e_min (eV): modes below it
    are left out of the thermodynamic sums; max_q_per_call: q-points per `snet_ph_dynmat` launch (a cap on its scratch).  extra /
    make_extra exactly as vibrations_batch, over the copy slots of the SUPERCELLS: make_extra(slot_system) -> extra, slot s holding a
    copy of the supercell of system slot_system[s].  The caller's arrays are not modified.

    Returns (results, info).  results[b]: the keys of SevenNetCalculator.compute_many for the undisplaced supercell (the model's
    values; per-atom energies as `atomic_energies`), `supercell` (the repeats), `supercell_positions` [N,3], `supercell_cell` [3,3],
    `force_constants` [m,N,3,3] (eV/A^2: [alpha, j, i, k], after the sum-rule correction if asked), `asr_defect` (before it),
    `qpoints` [n_q,3] with `eigenvalues` / `energies` (eV, signed) / `frequencies` (cm^-1) [n_q,3m], `hermiticity` [n_q] (max
    |R - R^H| before D(q) is symmetrised) and, with want_modes, `modes` [n_q,3m,m,3] complex (full-vector phase convention); with
    mesh: `mesh`, `dos_energies`, `dos` (states per eV and primitive cell) and `thermo` (`thermodynamics`); `status`: 'ok' or
    'failed' (a non-finite force: everything that follows from Phi is NaN).  info: `n_force_calls`, `copies_evaluated`, `launches`
    and `q_evaluated`.  Invalid input raises ValueError before any device work."""
    types, positions, n_at, cells, pbcs = validate_batch_inputs(types, positions, cells, pbcs, cutoff, engine.spec.num_species, n_atoms)
    masses, selected = validate_vib_inputs(n_at, masses, None, delta, nfree, max_atoms_per_call)
    repeats, q_list, mesh, temps = validate_phonon_inputs(n_at, cells, pbcs, supercells, qpoints, mesh, temperatures, symprec, e_min,
                                                          dos_bins, max_q_per_call)
    check_extra(extra, make_extra)
    B = len(n_at)
    a_ptr = np.concatenate([[0], np.cumsum(n_at)])
    positions = _as_host(positions, np.float64).reshape(-1, 3)
    sc = [build_supercell(types[a_ptr[b]:a_ptr[b + 1]], positions[a_ptr[b]:a_ptr[b + 1]], cells[b], repeats[b]) for b in range(B)]
    N = np.array([len(s[0]) for s in sc], np.int64)
    S = np.stack([s[2] for s in sc])
    pbc_sc = np.ones((B, 3), bool)
    plan = plan_copies(N, selected, nfree, int(max_atoms_per_call))
    slot = plan.slot_system
    if make_extra is not None:
        extra = make_extra(slot)
    forces = BatchForces(engine, np.concatenate([sc[b][0] for b in slot]), N[slot], S[slot], pbc_sc[slot], cutoff, extra)
    mesh_q = mesh_points(mesh) if mesh is not None else np.zeros((0, 3))
    q_frac = [np.concatenate([q_list[b], mesh_q]) for b in range(B)]
    q_cart = [2.0 * np.pi * (q_frac[b] @ np.linalg.inv(cells[b]).T) for b in range(B)]
    base = BaseCopies(want_atomic_virial)
    phi, asr, D, herm, status, info = phonon_loop(forces, plan, np.concatenate([s[1] for s in sc]), N, n_at, masses, S, q_cart,
                                                  delta=delta, acoustic=acoustic, symprec=symprec, max_q_per_call=int(max_q_per_call),
                                                  keeper=base, want_atomic_virial=want_atomic_virial)
    base = base.results(N, S, 'atomic_energies')
    results = []
    for b in range(B):
        res = base[b]
        n_path = len(q_list[b])
        res.update(supercell=repeats[b].copy(), supercell_positions=sc[b][1], supercell_cell=S[b].copy(), force_constants=phi[b],
                   asr_defect=float(asr[b]), qpoints=q_list[b].copy(), hermiticity=herm[b][:n_path].copy(),
                   status=VIB_STATUS_NAMES[0 if status[b] == 0 else 1])
        res.update(spectrum(D[b][:n_path], want_modes))
        if mesh is not None:
            e_mesh = spectrum(D[b][n_path:])['energies']
            centres, density = dos(e_mesh, dos_bins)
            res.update(mesh=mesh, dos_energies=centres, dos=density, thermo=thermodynamics(e_mesh, temps, e_min))
        results.append(res)
    return results, info
