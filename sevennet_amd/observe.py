"""Observables of `md_batch` accumulated on the device: the radial distribution function, the mean-square displacement and the
velocity autocorrelation function.

An `Observe` passed to `md_batch` (`SevenNetCalculator.md_many(..., observe=...)`) makes the MD loop sample (x_k, v_k) at every
step k that is a multiple of `every`: one `snet_obs_rdf` launch adds the sample's pair counts to a uint64 histogram, one
`snet_obs_correlate` launch adds, for every origin frame still within `lags` samples, the squared displacements and the velocity
products per kind (csrc/snet_observe.hip; the rules are written out in include/snet_hip.h and restated in tests/observe_ref.py).
Origin frames are kept in a ring of ceil(lags / origin_every) frames on the device, stored by a device-to-device copy.  Nothing
is read back while the loop runs; the accumulators come to the host after it, where `attach_observables` turns them into g(r),
MSD and VACF.  `diffusion_coefficient` and `vdos` are host helpers for what usually follows.  Units: A, fs, amu."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .batch import _pad_cells

MAX_KINDS = 8          # kinds per system (snet_obs_rdf, snet_obs_correlate)
MAX_HIST = 8192        # kinds^2 bins: the uint32 histogram of one workgroup in LDS
MAX_REACH = 4          # lattice shifts per axis
MAX_RING = 65535       # origin frames: the second grid dimension of snet_obs_correlate
TILE_ROWS = 32         # rows of a system per snet_obs_rdf workgroup
LIGHT_CM_PER_FS = 2.99792458e-5


@dataclass(frozen=True)
class Observe:
    """What `md_batch` samples.  every: sample every that many steps (steps // every + 1 samples, step 0 included).  rdf_rmax
    (A; None: no RDF) and rdf_bins: pair distances below rdf_rmax in rdf_bins equal bins.  lags (0: no MSD / VACF): lag 0 ..
    lags - 1 in units of one sample; origin_every: every that many samples a new time origin.  remove_com: displacements and
    velocities relative to the system's mass-weighted centre of mass of each frame (a system with held components is anchored
    and not corrected).  by_species: per species present in the system (False: one kind for all atoms)."""
    every: int
    rdf_rmax: Optional[float] = None
    rdf_bins: int = 100
    lags: int = 0
    origin_every: int = 1
    remove_com: bool = True
    by_species: bool = True


# ---------------------------------------------------------------------------------------------------- the ring, on the host
def ring_size(lags: int, origin_every: int) -> int:
    """origin frames that can be within `lags` samples at once: ceil(lags / origin_every)"""
    return -(-int(lags) // int(origin_every))


def live_origins(sample: int, lags: int, origin_every: int) -> List[Tuple[int, int]]:
    """[(slot, lag)] of the origins sample number `sample` is correlated with, by slot: origin q is sample q origin_every, sits in
    slot q % ring and is live while lag = sample - q origin_every < lags (the arithmetic of snet_obs_correlate)"""
    ring, q_last, out = ring_size(lags, origin_every), sample // origin_every, []
    for slot in range(ring):
        if q_last < slot:
            continue
        q = q_last - (q_last - slot) % ring
        lag = sample - q * origin_every
        if lag < lags:
            out.append((slot, lag))
    return out


def origin_counts(n_samples: int, lags: int, origin_every: int) -> np.ndarray:
    """int64 [lags]: how many (origin, sample) pairs of a run of n_samples samples have lag l"""
    n = np.zeros(lags, np.int64)
    for l in range(lags):   # origins q origin_every with q origin_every + l <= n_samples - 1
        if n_samples - 1 - l >= 0:
            n[l] = (n_samples - 1 - l) // origin_every + 1
    return n


# ---------------------------------------------------------------------------------------------------- host checks
def _is_int(v, low: int) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and v >= low


def validate_observe(obs: Observe) -> None:
    """the settings alone (ValueError)"""
    if not isinstance(obs, Observe):
        raise ValueError(f'observe = {obs!r}: an observe.Observe is required')
    for name, v, low in (('every', obs.every, 1), ('rdf_bins', obs.rdf_bins, 1), ('lags', obs.lags, 0), ('origin_every', obs.origin_every, 1)):
        if not _is_int(v, low):
            raise ValueError(f'observe: {name} = {v!r}, an integer >= {low} is required')
    if obs.rdf_rmax is not None:
        r = obs.rdf_rmax
        if isinstance(r, bool) or not isinstance(r, (int, float, np.floating, np.integer)) or not (r > 0 and math.isfinite(r)):
            raise ValueError(f'observe: rdf_rmax = {r!r}, a finite distance > 0 (A) is required')
    if obs.rdf_rmax is None and obs.lags == 0:
        raise ValueError('observe: neither rdf_rmax nor lags given, there is nothing to accumulate')
    if ring_size(obs.lags, obs.origin_every) > MAX_RING:
        raise ValueError(f'observe: lags = {obs.lags} with origin_every = {obs.origin_every} needs a ring of '
                         f'{ring_size(obs.lags, obs.origin_every)} origin frames, at most {MAX_RING} are kept (raise origin_every)')


def image_reach(cells: np.ndarray, pbcs: np.ndarray, r_max: float) -> np.ndarray:
    """int64 [B,3]: floor(r_max / height_k + 0.5) on periodic axes, 0 on open ones.  After the nearest-image reduction a
    fractional difference is at most 1/2, so an image within r_max is at most that many cells away."""
    inv = np.linalg.inv(_pad_cells(cells, pbcs, 1.0))
    per_height = np.linalg.norm(inv, axis=1)   # 1 / height_k: the length of column k of the inverse
    return np.where(pbcs, np.floor(r_max * per_height + 0.5), 0.0).astype(np.int64)


def observe_plan(obs: Observe, types: np.ndarray, n_at: np.ndarray, cells: np.ndarray, pbcs: np.ndarray) -> Dict[str, Any]:
    """Everything the accumulators need, from validated batch inputs (`batch.validate_batch_inputs`), on the host: the kinds of
    each system (species indices present, ascending; None with by_species False), kind int32 [N], kind_ptr int32 [B+1], and for
    the RDF sys_desc int32 [B,8], tile int32 [T,3], the padded cells and the caps of the launch.  ValueError names the system."""
    validate_observe(obs)
    B = len(n_at)
    a_ptr = np.concatenate([[0], np.cumsum(n_at)]).astype(np.int64)
    types = np.asarray(types, np.int64).reshape(-1)
    pbcs = np.asarray(pbcs, bool).reshape(B, 3)
    cells = np.asarray(cells, np.float64).reshape(B, 3, 3)
    kind = np.zeros(len(types), np.int32)
    kinds: List[Optional[np.ndarray]] = []
    n_kinds = np.ones(B, np.int64)
    for b in range(B):
        if not obs.by_species:
            kinds.append(None)
            continue
        t = types[a_ptr[b]:a_ptr[b + 1]]
        present = np.unique(t)
        if len(present) > MAX_KINDS:
            raise ValueError(f'system {b}: {len(present)} species, observables are kept for at most {MAX_KINDS} kinds per system '
                             '(pass by_species=False)')
        kind[a_ptr[b]:a_ptr[b + 1]] = np.searchsorted(present, t)
        kinds.append(present)
        n_kinds[b] = max(len(present), 1)
    plan: Dict[str, Any] = dict(obs=obs, a_ptr=a_ptr, kinds=kinds, n_kinds=n_kinds, kind=kind, pbcs=pbcs, cells=cells,
                                kind_ptr=np.concatenate([[0], np.cumsum(n_kinds)]).astype(np.int32))
    if obs.rdf_rmax is not None:
        bins = int(obs.rdf_bins)
        for b in range(B):
            if n_kinds[b] ** 2 * bins > MAX_HIST:
                raise ValueError(f'system {b}: {n_kinds[b]} kinds and {bins} bins need {n_kinds[b] ** 2 * bins} histogram words, at '
                                 f'most {MAX_HIST} fit (fewer bins, or by_species=False)')
        reach = image_reach(cells, pbcs, float(obs.rdf_rmax))
        if (reach > MAX_REACH).any():
            b, k = (int(x[0]) for x in np.nonzero(reach > MAX_REACH))
            raise ValueError(f'system {b}: rdf_rmax = {obs.rdf_rmax} A reaches {reach[b, k]} cells along axis {k}, at most {MAX_REACH} '
                             'are searched (use a supercell)')
        sizes = n_kinds ** 2 * bins
        off = np.concatenate([[0], np.cumsum(sizes)])
        desc = np.zeros((B, 8), np.int32)
        desc[:, 0], desc[:, 1] = n_kinds, off[:-1]
        desc[:, 2] = pbcs[:, 0] + 2 * pbcs[:, 1] + 4 * pbcs[:, 2]
        desc[:, 3:6] = reach
        tiles = [(b, r0, min(TILE_ROWS, int(n_at[b]) - r0)) for b in range(B) for r0 in range(0, int(n_at[b]), TILE_ROWS)]
        plan.update(bins=bins, dr=float(obs.rdf_rmax) / bins, count_ptr=off.astype(np.int64), sys_desc=desc,
                    tile=np.asarray(tiles, np.int32).reshape(-1, 3), kinds_max=int(n_kinds.max()), reach_max=int(reach.max()),
                    cells_padded=_pad_cells(cells, pbcs, 1.0))
    return plan


# ---------------------------------------------------------------------------------------------------- launches
def obs_rdf(pos: torch.Tensor, seg_ptr: torch.Tensor, kind: torch.Tensor, cell: torch.Tensor, sys_desc: torch.Tensor,
            tile: torch.Tensor, dr: float, bins: int, kinds_max: int, reach_max: int, counts: torch.Tensor) -> None:
    """one `snet_obs_rdf` launch on the current stream: the pair counts of this frame are added to counts (int64 [n_counts] on the
    device, read as the uint64 words of the C ABI).  pos fp64 [N,3], seg_ptr int32 [B+1], kind int32 [N], cell fp64 [B,9], sys_desc
    int32 [B,8], tile int32 [T,3] (include/snet_hip.h)"""
    N, B, T = int(pos.shape[0]), int(seg_ptr.numel()) - 1, int(tile.shape[0])
    i32 = torch.int32
    _lib.check_device_tensors('obs_rdf', pos, [(pos, torch.float64, (N, 3)), (seg_ptr, i32, (B + 1,)), (kind, i32, (N,)),
                                               (cell, torch.float64, (B, 9)), (sys_desc, i32, (B, 8)), (tile, i32, (T, 3)),
                                               (counts, torch.int64, (int(counts.numel()),))])
    P = _lib.ptr
    with torch.cuda.device(pos.device):
        _lib.check(_lib.load().snet_obs_rdf(P(pos), N, P(seg_ptr), B, P(kind), P(cell), P(sys_desc), P(tile), T, float(dr), int(bins),
                                            int(kinds_max), int(reach_max), P(counts), int(counts.numel()), _lib.stream()),
                   'snet_obs_rdf')


def obs_correlate(pos: torch.Tensor, vel: torch.Tensor, ring_pos: torch.Tensor, ring_vel: torch.Tensor, mass: torch.Tensor,
                  seg_ptr: torch.Tensor, kind: torch.Tensor, kind_ptr: torch.Tensor, sample: int, origin_every: int, lags: int,
                  remove_com: bool, msd_sum: torch.Tensor, vacf_sum: torch.Tensor, hold: Optional[torch.Tensor] = None) -> None:
    """one `snet_obs_correlate` launch on the current stream: sample number `sample` (pos, vel fp64 [N,3]) against the origins in
    ring_pos / ring_vel (fp64 [ring,N,3], ring = ring_size(lags, origin_every)); msd_sum / vacf_sum (fp64 [kinds,lags], kinds =
    kind_ptr[-1]) are added to.  The origin of this sample, if it is one, must be in its slot already."""
    N, B, R, K = int(pos.shape[0]), int(seg_ptr.numel()) - 1, ring_size(lags, origin_every), int(msd_sum.shape[0])
    f64, i32 = torch.float64, torch.int32
    want = [(pos, f64, (N, 3)), (vel, f64, (N, 3)), (ring_pos, f64, (R, N, 3)), (ring_vel, f64, (R, N, 3)), (mass, f64, (N,)),
            (seg_ptr, i32, (B + 1,)), (kind, i32, (N,)), (kind_ptr, i32, (B + 1,)), (msd_sum, f64, (K, int(lags))),
            (vacf_sum, f64, (K, int(lags)))]
    if hold is not None:
        want.append((hold, i32, (N,)))
    _lib.check_device_tensors('obs_correlate', pos, want)
    P = _lib.ptr
    with torch.cuda.device(pos.device):
        _lib.check(_lib.load().snet_obs_correlate(P(pos), P(vel), P(ring_pos), P(ring_vel), P(mass), P(hold), N, P(seg_ptr), B, P(kind),
                                                  P(kind_ptr), K, int(sample), int(origin_every), R, int(lags), int(bool(remove_com)),
                                                  P(msd_sum), P(vacf_sum), _lib.stream()), 'snet_obs_correlate')


class Accumulator:
    """The device state of one run: descriptors, histogram, ring and sums.  `sample(pos, vel)` issues the launches of one sample
    on the current stream; `to_host()` is the one transfer."""

    def __init__(self, plan: Dict[str, Any], mass: torch.Tensor, seg_ptr: torch.Tensor, hold: Optional[torch.Tensor], dev):
        up = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a, dtype)).to(dev)  # noqa: E731
        obs = plan['obs']
        self.plan, self.obs, self.mass, self.seg_ptr, self.hold = plan, obs, mass, seg_ptr, hold
        self.n_samples = 0
        N = int(mass.shape[0])
        self.kind = up(plan['kind'], np.int32)
        self.counts = None
        if obs.rdf_rmax is not None:
            self.cell = up(plan['cells_padded'].reshape(-1, 9), np.float64)
            self.sys_desc, self.tile = up(plan['sys_desc'], np.int32), up(plan['tile'], np.int32)
            self.counts = torch.zeros(int(plan['count_ptr'][-1]), dtype=torch.int64, device=dev)
        self.msd_sum = self.vacf_sum = None
        if obs.lags > 0:
            R, K = ring_size(obs.lags, obs.origin_every), int(plan['kind_ptr'][-1])
            self.kind_ptr = up(plan['kind_ptr'], np.int32)
            self.ring_pos = torch.zeros(R, N, 3, dtype=torch.float64, device=dev)
            self.ring_vel = torch.zeros_like(self.ring_pos)
            self.msd_sum = torch.zeros(K, obs.lags, dtype=torch.float64, device=dev)
            self.vacf_sum = torch.zeros_like(self.msd_sum)

    def sample(self, pos: torch.Tensor, vel: torch.Tensor) -> None:
        obs, p, s = self.obs, self.plan, self.n_samples
        if self.counts is not None:
            obs_rdf(pos, self.seg_ptr, self.kind, self.cell, self.sys_desc, self.tile, p['dr'], p['bins'], p['kinds_max'],
                    p['reach_max'], self.counts)
        if self.msd_sum is not None:
            if s % obs.origin_every == 0:   # a new origin: into its slot before the launch that reads it at lag 0
                slot = (s // obs.origin_every) % int(self.ring_pos.shape[0])
                self.ring_pos[slot].copy_(pos)
                self.ring_vel[slot].copy_(vel)
            obs_correlate(pos, vel, self.ring_pos, self.ring_vel, self.mass, self.seg_ptr, self.kind, self.kind_ptr, s,
                          obs.origin_every, obs.lags, obs.remove_com, self.msd_sum, self.vacf_sum, self.hold)
        self.n_samples = s + 1

    def to_host(self) -> Dict[str, Any]:
        h = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return dict(n_samples=self.n_samples, counts=h(self.counts), msd_sum=h(self.msd_sum), vacf_sum=h(self.vacf_sum))


# ---------------------------------------------------------------------------------------------------- post-processing
def attach_observables(results: List[Dict[str, Any]], plan: Dict[str, Any], acc: Dict[str, Any], dt: float) -> List[Dict[str, Any]]:
    """`observables` into each system's results dict, from the accumulators on the host (`Accumulator.to_host`):
    every, n_samples, kinds (species indices, None with by_species False); with an RDF `rdf` = dict(edges [bins+1], r [bins] (bin
    centres), counts int64 [S,S,bins], g [S,S,bins] = counts / (n_samples N_a (N_b / V) shell volume), None for a system that is not
    periodic along all three axes); with lags `lag_times` (fs), `n_origins` int64 [lags], `msd` [S,lags] and `msd_all` [lags]
    (A^2 per atom), `vacf` [S,lags] and `vacf_all` (A^2/fs^2 per atom); NaN where a lag has no origin yet."""
    obs, a_ptr, n_samples = plan['obs'], plan['a_ptr'], int(acc['n_samples'])
    for b, res in enumerate(results):
        S = int(plan['n_kinds'][b])
        lo, hi = int(a_ptr[b]), int(a_ptr[b + 1])
        per_kind = np.bincount(plan['kind'][lo:hi], minlength=S).astype(np.float64)
        out: Dict[str, Any] = dict(every=int(obs.every), n_samples=n_samples,
                                   kinds=None if plan['kinds'][b] is None else plan['kinds'][b].copy())
        if acc['counts'] is not None:
            bins = plan['bins']
            c0 = int(plan['count_ptr'][b])
            counts = acc['counts'][c0:c0 + S * S * bins].reshape(S, S, bins).copy()
            edges = plan['dr'] * np.arange(bins + 1)
            g = None
            if plan['pbcs'][b].all():
                shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
                volume = abs(np.linalg.det(plan['cells'][b]))
                with np.errstate(divide='ignore', invalid='ignore'):
                    g = counts / (n_samples * per_kind[:, None, None] * (per_kind[None, :, None] / volume) * shell[None, None, :])
            out['rdf'] = dict(edges=edges, r=0.5 * (edges[1:] + edges[:-1]), counts=counts, g=g)
        if acc['msd_sum'] is not None:
            k0 = int(plan['kind_ptr'][b])
            n_or = origin_counts(n_samples, obs.lags, obs.origin_every)
            out['lag_times'] = np.arange(obs.lags) * (float(obs.every) * float(dt))
            out['n_origins'] = n_or
            origins = np.where(n_or > 0, n_or, np.nan)   # (NaN: no origin has reached that lag)
            for name, key in (('msd', 'msd_sum'), ('vacf', 'vacf_sum')):
                sums = acc[key][k0:k0 + S]
                out[name] = sums / (origins[None, :] * per_kind[:, None])
                out[name + '_all'] = sums.sum(0) / (origins * float(hi - lo))
        res['observables'] = out
    return results


def diffusion_coefficient(msd, lag_times, fit: Tuple[float, float]) -> Tuple[float, float]:
    """(D, residual): D = slope / 6 (A^2/fs) of the least-squares line through msd over t_lo <= lag_times <= t_hi, and the root mean
    square of what the line leaves (A^2)"""
    msd, t = np.asarray(msd, np.float64), np.asarray(lag_times, np.float64)
    if msd.shape != t.shape or msd.ndim != 1:
        raise ValueError(f'msd of shape {msd.shape} and lag_times of shape {t.shape}: two arrays [lags] are required')
    sel = (t >= fit[0]) & (t <= fit[1]) & np.isfinite(msd)
    if sel.sum() < 2:
        raise ValueError(f'fit = {fit}: fewer than two lags in the window')
    A = np.stack([t[sel], np.ones(int(sel.sum()))], 1)
    coef = np.linalg.lstsq(A, msd[sel], rcond=None)[0]
    return float(coef[0]) / 6.0, float(np.sqrt(np.mean((A @ coef - msd[sel]) ** 2)))


def vdos(vacf, dt_sample: float, n_freq: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(wavenumbers in 1/cm, spectrum): the one-sided cosine transform 2 dt sum_t w_t vacf[t] cos(2 pi f t dt), trapezoid weights
    (w = 1/2 at both ends), at n_freq (default: len(vacf)) frequencies f from 0 to the Nyquist frequency 1 / (2 dt_sample)"""
    c = np.asarray(vacf, np.float64)
    if c.ndim != 1 or len(c) < 2 or not dt_sample > 0:
        raise ValueError('vdos: a vacf of at least two lags and a sample spacing > 0 (fs) are required')
    n = len(c)
    m = n if n_freq is None else int(n_freq)
    f = np.arange(m) / (2.0 * max(m - 1, 1) * dt_sample)
    w = np.ones(n)
    w[0] = w[-1] = 0.5
    spectrum = 2.0 * dt_sample * (np.cos(2.0 * np.pi * np.outer(f, np.arange(n) * dt_sample)) @ (w * c))
    return f / LIGHT_CM_PER_FS, spectrum
