"""Batched nudged elastic band: many bands relax at once, positions and optimizer state on the device from the first step to
the last.

A band is M images of the same atoms in the same cell; its two endpoints stay where they are and its M - 2 interior images
move.  `neb_batch` relaxes B bands at once: per step one batched evaluation of all moving images (sevennet_amd.batch), one
`snet_neb_forces` launch (csrc/snet_neb.hip: one workgroup per moving image, fp64, fixed summation order) that turns the true
forces and the image energies into NEB forces, and one `snet_fire_step` launch with ONE SEGMENT PER BAND -- the single FIRE that
ASE runs over `FIRE(NEB(images))`: all moving images of a band share one dt, one alpha, one max_step clip and one fmax test.
The only thing read back per step is the number of bands still active; converged bands leave the batch as the systems of
`relax.fire_loop` do.

The rule -- improved tangent (Henkelman, Jonsson, J. Chem. Phys. 113, 9978 (2000)), springs along the tangent, climbing image
(Henkelman, Uberuaga, Jonsson, J. Chem. Phys. 113, 9901 (2000)) -- is written out in include/snet_hip.h (snet_neb_forces) and
restated in fp64 numpy in tests/neb_ref.py.  Displacements between neighbouring images are taken through the minimum-image
form mic(d): s = d inv(cell), s_k -= rint(s_k) on the periodic axes, d = s cell, which is the shortest image whenever the true
displacement is shorter than half the smallest face-to-face height of the cell (|s_k| <= |d| / h_k).  That is the documented
domain, not something the code checks: neighbouring images of a band are expected to be closer than that.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .batch import BatchForces, _pad_cells, batch_results, device_positions, to_device, validate_batch_inputs
from .relax import RepackBook, check_fire_params, fire_step

NEB_STATUS_NAMES = ('steps', 'converged', 'failed')   # 0: still running at the step cap; 2: the force kernel's guard switched the band off


def mic_cells(cells, pbcs) -> Tuple[np.ndarray, np.ndarray]:
    """(cells [B,3,3] with the zero rows of open axes padded as batch._pad_cells pads them, their inverses [B,3,3]): the matrices
    of the minimum-image form.  ValueError names a band whose padded cell is singular."""
    cells = np.asarray(cells, np.float64).reshape(-1, 3, 3)
    pbcs = np.broadcast_to(np.asarray(pbcs, bool).reshape(-1, 3), (len(cells), 3))
    padded = _pad_cells(cells, pbcs, 1.0)   # (the length of a padded row does not matter: open axes are not wrapped)
    det = np.linalg.det(padded)
    if (np.abs(det) <= 1e-12).any():
        b = int(np.nonzero(np.abs(det) <= 1e-12)[0][0])
        raise ValueError(f'band {b}: singular cell {cells[b].tolist()} (pbc {pbcs[b].tolist()})')
    return padded, np.linalg.inv(padded)


def mic(d: np.ndarray, cell, pbc) -> np.ndarray:
    """minimum-image form of the displacements d [...,3] (host, fp64): the shortest image whenever |d| is below half the
    smallest height of the cell; without a periodic axis d itself"""
    pbc = np.asarray(pbc, bool).reshape(3)
    d = np.asarray(d, np.float64)
    if not pbc.any():
        return d.copy()
    padded, inv = mic_cells(np.asarray(cell, np.float64).reshape(1, 3, 3), pbc)
    s = d @ inv[0]
    s[..., pbc] -= np.rint(s[..., pbc])
    return s @ padded[0]


def interpolate_band(initial, final, n_images: int, cell=None, pbc=(False, False, False)) -> np.ndarray:
    """[n_images, n, 3]: both endpoints (bit for bit) and n_images - 2 images between them, linear along mic(final - initial), so
    an atom that hops through a periodic face takes the short way (the images are not wrapped back into the cell)"""
    initial, final = np.asarray(initial, np.float64), np.asarray(final, np.float64)
    if initial.ndim != 2 or initial.shape[1] != 3 or initial.shape != final.shape:
        raise ValueError(f'interpolate_band: endpoints of shape [n,3] are required, got {initial.shape} and {final.shape}')
    if int(n_images) != n_images or n_images < 2:
        raise ValueError(f'n_images = {n_images}: at least the two endpoints are required')
    d = mic(final - initial, np.zeros((3, 3)) if cell is None else cell, pbc)
    band = initial[None] + np.linspace(0.0, 1.0, int(n_images))[:, None, None] * d[None]
    band[0], band[-1] = initial, final
    return band


def neb_forces(pos: torch.Tensor, forces: torch.Tensor, energy: torch.Tensor, seg_ptr: torch.Tensor, img_ptr: torch.Tensor,
               pos_end: torch.Tensor, end_ptr: torch.Tensor, e_end: torch.Tensor, cells: torch.Tensor, inv_cells: torch.Tensor,
               pbc: torch.Tensor, k: torch.Tensor, active: torch.Tensor, status: torch.Tensor, f_neb: torch.Tensor,
               imax: torch.Tensor, *, climb: bool = False, forces_extra: Optional[torch.Tensor] = None,
               energy_extra: Optional[torch.Tensor] = None, fixed: Optional[torch.Tensor] = None) -> None:
    """one `snet_neb_forces` launch on the current stream; every tensor on the device (dtypes as the C ABI: pos / forces_extra /
    energy / energy_extra / pos_end / e_end / cells / inv_cells / k / f_neb fp64, forces fp32, the rest int32).  Writes f_neb and
    imax, and active / status of a band whose input is not finite."""
    N, n_img, B, n_end = int(pos.shape[0]), int(seg_ptr.numel()) - 1, int(img_ptr.numel()) - 1, int(pos_end.shape[0])
    f64, i32 = torch.float64, torch.int32
    want = [(pos, f64, (N, 3)), (forces, torch.float32, (N, 3)), (energy, f64, (n_img,)), (seg_ptr, i32, (n_img + 1,)),
            (img_ptr, i32, (B + 1,)), (pos_end, f64, (n_end, 3)), (end_ptr, i32, (B + 1,)), (e_end, f64, (B, 2)), (cells, f64, (B, 9)),
            (inv_cells, f64, (B, 9)), (pbc, i32, (B, 3)), (k, f64, (B,)), (active, i32, (B,)), (status, i32, (B,)), (f_neb, f64, (N, 3)),
            (imax, i32, (B,))]
    if forces_extra is not None:
        want.append((forces_extra, f64, (N, 3)))
    if energy_extra is not None:
        want.append((energy_extra, f64, (n_img,)))
    if fixed is not None:
        want.append((fixed, i32, (N,)))
    _lib.check_device_tensors('neb_forces', pos, want)
    P = _lib.ptr
    with torch.cuda.device(pos.device):
        _lib.check(_lib.load().snet_neb_forces(
            P(pos), P(forces), P(forces_extra), P(energy), P(energy_extra), N, P(seg_ptr), n_img, P(img_ptr), B, P(pos_end), P(end_ptr),
            n_end, P(e_end), P(cells), P(inv_cells), P(pbc), P(fixed), P(k), int(bool(climb)), P(active), P(status), P(f_neb), P(imax),
            _lib.stream()), 'snet_neb_forces')


class BandLayout:
    """Where the images of B bands sit in the flattened list of all images (band after band, endpoints included), on the host:
    n_images [B] (M_b), n_atoms [B] (n_b), the first image `img0` [B+1] and the first flat row `row0` [sum M_b + 1] of each."""

    def __init__(self, n_images, n_atoms_per_image):
        self.M = np.asarray(n_images, np.int64).reshape(-1)
        per_image = np.asarray(n_atoms_per_image, np.int64).reshape(-1)
        if (self.M < 3).any():
            b = int(np.nonzero(self.M < 3)[0][0])
            raise ValueError(f'band {b}: {int(self.M[b])} images, but a band needs two endpoints and at least one image between them')
        if int(self.M.sum()) != len(per_image):
            raise ValueError(f'the bands have {int(self.M.sum())} images in all, but the force call was built over {len(per_image)} systems')
        self.B = len(self.M)
        self.img0 = np.concatenate([[0], np.cumsum(self.M)])
        self.row0 = np.concatenate([[0], np.cumsum(per_image)])
        self.n = per_image[self.img0[:-1]]
        for b in range(self.B):
            if (per_image[self.img0[b]:self.img0[b + 1]] != self.n[b]).any():
                raise ValueError(f'band {b}: its images do not all have the same number of atoms')
        self.m = self.M - 2   # moving images

    def interior_images(self, bands) -> np.ndarray:
        return np.concatenate([np.arange(self.img0[b] + 1, self.img0[b + 1] - 1) for b in bands])

    def end_images(self, bands) -> np.ndarray:
        return np.concatenate([[self.img0[b], self.img0[b + 1] - 1] for b in bands])

    def rows(self, images) -> np.ndarray:
        return np.concatenate([np.arange(self.row0[j], self.row0[j + 1]) for j in images])

    def ptr(self, bands, per_band) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(np.asarray(per_band, np.int64)[np.asarray(bands, np.int64)])])


def _fixed_rows(layout: BandLayout, fixed) -> Optional[np.ndarray]:
    """int32 [moving rows of all bands]: 1 for a fixed atom, from one bool mask [n_b] per band (entries may be None)"""
    if fixed is None or all(f is None for f in fixed):
        return None
    out = []
    for b in range(layout.B):
        mask = np.zeros(layout.n[b], np.int32) if fixed[b] is None else np.asarray(fixed[b], bool).astype(np.int32)
        out.append(np.tile(mask, layout.m[b]))
    return np.concatenate(out)


def neb_loop(forces, n_images, positions, cells, pbcs, *, fmax: float, steps: int, repack_below: float, params: dict, k,
             climb: bool = False, fixed=None):
    """The band relaxation loop.  forces: a BatchForces over the flattened list of all images of all bands (band after band,
    endpoints included), or any object with its call interface, as relax.fire_cell_loop documents it: (pos, ids) -> (graph with
    `seg_ptr`, output with `forces` fp32 [N,3] and `energy_per_system` fp64 [b], extra forces fp64 [N,3] or None, extra
    energies fp64 [b] or None), its counters, `n_atoms` (per image) and `engine.dev`.  n_images [B]: M_b; positions: the flat
    [sum M_b n_b, 3] positions of all images; cells [B,3,3], pbcs [B,3], k [B] and fixed (None, or one bool mask [n_b] or None
    per band): per band.  Before the loop one evaluation of the 2 B endpoints, whose energies stay on the device.  Per step one
    evaluation of the moving images of the bands still in the batch, one `snet_neb_forces`, one `snet_fire_step` with the
    bands as its segments (its `forces` a zero tensor, its `forces_extra` the NEB forces) and one readback (n_active).  An
    extra term that returns forces without energies raises ValueError: the tangent needs the energies.
    -> (positions fp64 [N,3] of all images on the device in the caller's order, n_steps [B], status [B] (0 step cap, 1
    converged: the largest atomic NEB force of the band below fmax, 2 failed: a non-finite energy, force or displacement, the
    band is returned as it was before that step), info)"""
    dev = forces.engine.dev
    lay = BandLayout(n_images, forces.n_atoms)
    B = lay.B
    book = RepackBook(lay.m * lay.n)
    padded, inv = mic_cells(cells, pbcs)
    pbcs = np.array(np.broadcast_to(np.asarray(pbcs, bool).reshape(-1, 3), (B, 3)))
    fixed_h = _fixed_rows(lay, fixed)
    f64, i32 = torch.float64, torch.int32
    status_all, n_launches = np.zeros(B, np.int64), 0

    with torch.cuda.device(dev):
        pos_all = device_positions(positions, dev).clone()
        every = np.arange(B)
        moving_rows = to_device(lay.rows(lay.interior_images(every)), torch.int64, dev)
        end_ids = lay.end_images(every)
        pos_end = pos_all[to_device(lay.rows(end_ids), torch.int64, dev)]
        _, out, fx, ex = forces(pos_end, end_ids)
        if fx is not None and ex is None:
            raise ValueError('neb: the extra term returned forces without energies, but the tangent of a band is chosen by the '
                             'energies of its images: an `extra` must return (forces, energy_per_system)')
        e_end = (out['energy_per_system'].to(f64) + (0.0 if ex is None else ex)).reshape(B, 2).contiguous()
        pos = pos_all[moving_rows]
        N = int(pos.shape[0])
        vel = torch.zeros_like(pos)
        zero32 = torch.zeros(N, 3, dtype=torch.float32, device=dev)   # the `forces` of snet_fire_step: all of the force is f_neb
        f_neb = torch.zeros(N, 3, dtype=f64, device=dev)
        fixed_d = None if fixed_h is None else to_device(fixed_h, i32, dev)
        k_d, cells_d = to_device(k, f64, dev).reshape(B), to_device(padded.reshape(B, 9), f64, dev)
        inv_d, pbc_d = to_device(inv.reshape(B, 9), f64, dev), to_device(pbcs, i32, dev)
        dt = torch.full((B,), float(params['dt_start']), dtype=f64, device=dev)
        alpha = torch.full((B,), float(params['alpha_start']), dtype=f64, device=dev)
        n_pos, n_steps, status, imax = (torch.zeros(B, dtype=i32, device=dev) for _ in range(4))
        active = torch.ones(B, dtype=i32, device=dev)
        fmax_sys = torch.zeros(B, dtype=f64, device=dev)
        n_active = torch.zeros(1, dtype=i32, device=dev)

        def tables():   # of the bands in the batch: their moving images' ids, and the three offset arrays on the device
            ids = book.ids
            return (lay.interior_images(ids), to_device(lay.ptr(ids, lay.m), i32, dev), to_device(book.seg_ptr(), i32, dev),
                    to_device(lay.ptr(ids, 2 * lay.n), i32, dev))

        def note(status_h, active_h, only_finished):
            for slot, b in enumerate(book.ids):
                if not (only_finished and active_h[slot]):
                    status_all[b] = 2 if status_h[slot] >= 2 else (0 if active_h[slot] else 1)

        img_ids, img_ptr, band_ptr, end_ptr = tables()
        for _ in range(int(steps)):
            g, out, fx, ex = forces(pos, img_ids)
            neb_forces(pos, out['forces'], out['energy_per_system'], g.seg_ptr, img_ptr, pos_end, end_ptr, e_end, cells_d, inv_d, pbc_d,
                       k_d, active, status, f_neb, imax, climb=climb, forces_extra=fx, energy_extra=ex, fixed=fixed_d)
            fire_step(pos, vel, zero32, band_ptr, dt, alpha, n_pos, active, n_steps, fmax_sys, n_active, fmax, params, f_neb)
            n_launches += 1
            left = int(n_active.item())   # the one readback of the step
            if left == 0:
                break
            if book.wants_repack(left, len(book.ids), repack_below):
                act_h, st_h, status_h = torch.stack([active, n_steps, status]).cpu().numpy()
                note(status_h, act_h, only_finished=True)
                old_end = lay.ptr(book.ids, 2 * lay.n)
                keep, rows = book.repack(pos, act_h, st_h)
                rows_d, keep_d = to_device(rows, torch.int64, dev), to_device(keep, torch.int64, dev)
                end_rows = to_device(np.concatenate([np.arange(old_end[s], old_end[s + 1]) for s in keep]), torch.int64, dev)
                pos, vel, pos_end = pos[rows_d], vel[rows_d], pos_end[end_rows]   # (gathers copy: the stored slices keep the old buffer)
                fixed_d = None if fixed_d is None else fixed_d[rows_d]
                zero32, f_neb = zero32[:len(rows)], f_neb[:len(rows)]
                k_d, cells_d, inv_d, pbc_d, e_end, dt, alpha, n_pos, active, n_steps, status, imax, fmax_sys = (
                    t[keep_d] for t in (k_d, cells_d, inv_d, pbc_d, e_end, dt, alpha, n_pos, active, n_steps, status, imax, fmax_sys))
                img_ids, img_ptr, band_ptr, end_ptr = tables()
        act_h, st_h, status_h = torch.stack([active, n_steps, status]).cpu().numpy()
        note(status_h, act_h, only_finished=False)
        book.store(pos, act_h, st_h, only_finished=False)
        pos_all[moving_rows] = torch.cat(book.positions)
    info = dict(n_force_calls=forces.n_force_calls, n_repacks=book.n_repacks, system_steps_evaluated=forces.system_steps_evaluated,
                fire_launches=n_launches)
    return pos_all, book.n_steps.copy(), status_all, info


def _check_bands(types_list, images_list, cells, pbcs, k, fixed_list):
    """the band-level arguments of `neb_batch` on the host (ValueError names the band): -> (images as fp64 arrays [M_b,n_b,3],
    cells [B,3,3], pbcs [B,3], k [B], fixed as bool masks or None)"""
    if not isinstance(images_list, (list, tuple)) or not isinstance(types_list, (list, tuple)) or len(images_list) == 0:
        raise ValueError('neb: per-band lists of species arrays and of image arrays [M,n,3] are required (and at least one band)')
    B = len(images_list)
    if len(types_list) != B:
        raise ValueError(f'{len(types_list)} species arrays but {B} bands')
    images = []
    for b, im in enumerate(images_list):
        im = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if im.dtype == object or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f'band {b}: images of shape [M,n,3] are required, got {im.shape}')
        if im.shape[0] < 3:
            raise ValueError(f'band {b}: {im.shape[0]} images, but a band needs two endpoints and at least one image between them')
        n_types = int(np.asarray(types_list[b]).reshape(-1).shape[0])
        if im.shape[1] != n_types or n_types == 0:
            raise ValueError(f'band {b}: {n_types} species but images of {im.shape[1]} atoms')
        images.append(np.ascontiguousarray(im, np.float64))
    cells = np.asarray(cells, np.float64)
    if cells.size != 9 * B:
        raise ValueError(f'{B} bands but cells of shape {cells.shape}')
    cells = cells.reshape(B, 3, 3)
    pbcs = np.asarray(pbcs, bool)
    if pbcs.size == 3:
        pbcs = np.broadcast_to(pbcs.reshape(1, 3), (B, 3))
    if pbcs.size != 3 * B:
        raise ValueError(f'{B} bands but pbc of shape {pbcs.shape}')
    pbcs = np.ascontiguousarray(pbcs.reshape(B, 3))
    try:
        k_arr = np.asarray(k, np.float64).reshape(-1)
    except (TypeError, ValueError):
        k_arr = np.full(1, np.nan)
    if k_arr.size == 1:
        k_arr = np.full(B, k_arr[0])
    if k_arr.size != B:
        raise ValueError(f'k: one spring constant, or one per band ({B}), is required, got {k_arr.size}')
    bad = ~(np.isfinite(k_arr) & (k_arr > 0))
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError(f'band {b}: spring constant k = {k_arr[b]}: a finite positive value in eV/A^2 is required')
    fixed = None
    if fixed_list is not None:
        if len(fixed_list) != B:
            raise ValueError(f'fixed_list has {len(fixed_list)} entries but there are {B} bands')
        fixed = []
        for b, f in enumerate(fixed_list):
            n = images[b].shape[1]
            if f is None:
                fixed.append(None)
                continue
            f = np.asarray(f)
            if f.dtype == bool:
                if f.shape != (n,):
                    raise ValueError(f'band {b}: a fixed mask of shape ({n},) is required, got {f.shape}')
                fixed.append(f.copy())
                continue
            if f.size and (not np.issubdtype(f.dtype, np.integer) or f.ndim != 1):
                raise ValueError(f'band {b}: fixed atoms are given as a bool mask or a list of atom indices')
            f = f.astype(np.int64).reshape(-1)
            if ((f < 0) | (f >= n)).any():
                raise ValueError(f'band {b}: fixed atom index {int(f[(f < 0) | (f >= n)][0])} is out of range (the band has {n} atoms)')
            mask = np.zeros(n, bool)
            mask[f] = True
            fixed.append(mask)
    return images, cells, pbcs, k_arr, fixed


def neb_batch(engine, types_list, images_list, cells, pbcs, *, cutoff: float, fmax: float = 0.05, steps: int = 500, k=0.1,
              climb: bool = False, fixed_list=None, repack_below: float = 0.5, extra: Optional[Callable] = None,
              want_atomic_virial: bool = False, **fire) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """Relax B nudged elastic bands with FIRE until the largest atomic NEB force of each is below `fmax` (eV/A) or `steps` steps
    are done.

    engine: a HipForceEngine.  types_list[b]: species indices [n_b]; images_list[b]: [M_b, n_b, 3] with M_b >= 3, the first and
    the last image being the band's fixed endpoints (`interpolate_band` makes a starting band); cells [B,3,3], pbcs [B,3] (or
    one [3]): per band.  k: the spring constant in eV/A^2, one value or one per band.  climb: the interior image of highest
    energy climbs (its force along the tangent is reversed and it feels no spring).  Two-stage use is a second call with the
    first call's positions: a plain band first, then climb=True; no further API is needed.  fixed_list[b]: a bool mask [n_b] or
    a list of atom indices that do not move in any image (entries may be None).  repack_below: as relax_batch, in whole bands.
    extra: as batch.BatchForces, over the flattened list of all images (band after band), and it must return energies too;
    fire: relax.FIRE_DEFAULTS overrides.  The caller's arrays are not modified.  Neighbouring images must be closer than half
    the smallest cell height (module docstring).

    Returns (results, info).  results[b]: `images`, a list of M_b dicts with the keys of SevenNetCalculator.compute_many plus
    `positions` [n_b,3] fp64, from ONE batched evaluation of all images of all bands at the returned positions, endpoints
    included (the model's values; an `extra` term is not in them; want_atomic_virial adds `stresses`); `converged`, `n_steps`
    (the moves made) and `status`: 'converged', 'steps' (the step cap) or 'failed' (a non-finite energy, force or displacement: the band is returned as it was
    before that step); `neb_fmax`: the largest atomic NEB force at the returned positions, from one more force-kernel launch on
    that evaluation (NaN where it is not finite); `imax`: the index into `images` of the interior image of highest energy;
    `barrier` = max(E) - E[0] and `barrier_reverse` = max(E) - E[-1] over all images of the band.  neb_fmax, imax and the
    barriers include the extra term.  info: the counters of relax_batch.  Invalid input raises ValueError before any device
    work."""
    params = check_fire_params(fmax, steps, repack_below, fire)
    images, cells, pbcs, k_arr, fixed = _check_bands(types_list, images_list, cells, pbcs, k, fixed_list)
    B = len(images)
    M = np.array([im.shape[0] for im in images], np.int64)
    mic_cells(cells, pbcs)   # singular cells, by band
    band_of = np.repeat(np.arange(B), M)
    types, positions, n_at, cells_img, pbcs_img = validate_batch_inputs(
        [np.asarray(types_list[b]).reshape(-1) for b in band_of], [im[j] for im in images for j in range(im.shape[0])],
        cells[band_of], pbcs[band_of], cutoff, engine.spec.num_species)
    forces = BatchForces(engine, types, n_at, cells_img, pbcs_img, cutoff, extra)
    final, n_steps, status, info = neb_loop(forces, M, positions, cells, pbcs, fmax=fmax, steps=steps, repack_below=repack_below,
                                            params=params, k=k_arr, climb=climb, fixed=fixed)
    g, out, fx, ex = forces(final, want_atomic_virial=want_atomic_virial)
    info['n_force_calls'] = forces.n_force_calls
    flat = batch_results(g, out, cells_img, want_atomic_virial)
    dev = final.device
    lay = BandLayout(M, n_at)
    every = np.arange(B)
    f64, i32 = torch.float64, torch.int32

    with torch.cuda.device(dev):   # the NEB forces of the returned band: one launch on the evaluation above, every band active
        e_tot = out['energy_per_system'].to(f64) + (0.0 if ex is None else ex)
        inner, ends = lay.interior_images(every), lay.end_images(every)
        rows = to_device(lay.rows(inner), torch.int64, dev)
        padded, inv = mic_cells(cells, pbcs)
        fixed_h = _fixed_rows(lay, fixed)
        f_neb = torch.zeros(len(rows), 3, dtype=f64, device=dev)
        active, status_d, imax = torch.ones(B, dtype=i32, device=dev), torch.zeros(B, dtype=i32, device=dev), torch.zeros(B, dtype=i32, device=dev)
        band_ptr = lay.ptr(every, lay.m * lay.n)
        neb_forces(final[rows], out['forces'][rows].contiguous(), e_tot[to_device(inner, torch.int64, dev)].contiguous(),
                   to_device(np.concatenate([[0], np.cumsum(n_at[inner])]), i32, dev), to_device(lay.ptr(every, lay.m), i32, dev),
                   final[to_device(lay.rows(ends), torch.int64, dev)], to_device(lay.ptr(every, 2 * lay.n), i32, dev),
                   e_tot[to_device(ends, torch.int64, dev)].reshape(B, 2).contiguous(), to_device(padded.reshape(B, 9), f64, dev),
                   to_device(inv.reshape(B, 9), f64, dev), to_device(pbcs, i32, dev), to_device(k_arr, f64, dev), active, status_d, f_neb,
                   imax, climb=climb, forces_extra=None if fx is None else fx[rows].contiguous(),
                   fixed=None if fixed_h is None else to_device(fixed_h, i32, dev))
        norms = (f_neb * f_neb).sum(1).sqrt()
        neb_fmax = torch.stack([norms[int(band_ptr[b]):int(band_ptr[b + 1])].max() for b in range(B)]).cpu().numpy()
        imax_h, ok_h = imax.cpu().numpy(), status_d.cpu().numpy() == 0
        e_h, pos_h = e_tot.cpu().numpy(), final.cpu().numpy()
    results = []
    for b in range(B):
        j0, j1 = int(lay.img0[b]), int(lay.img0[b + 1])
        band = flat[j0:j1]
        for j, res in zip(range(j0, j1), band):
            res['positions'] = pos_h[int(lay.row0[j]):int(lay.row0[j + 1])].copy()
        e = e_h[j0:j1]
        results.append(dict(images=band, converged=bool(status[b] == 1), n_steps=int(n_steps[b]), status=NEB_STATUS_NAMES[int(status[b])],
                            neb_fmax=float(neb_fmax[b]) if ok_h[b] else float('nan'), imax=int(imax_h[b]) + 1,
                            barrier=float(e.max() - e[0]), barrier_reverse=float(e.max() - e[-1])))
    return results, info
