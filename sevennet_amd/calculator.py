"""ASE-facing host of the HIP force engine: drop-in for `sevenn.calculator.SevenNetCalculator`.

Keeps the reference's calculator surface (sevenn/calculator.py:20-233):
same constructor keywords, `implemented_properties`, result keys, units and sign
conventions
  energy / free_energy  eV
  energies              per-atom eV
  forces                eV/A  [N,3]
  stress                eV/A^3, Voigt (xx,yy,zz,yz,xz,xy) = -model_stress[[0,1,2,4,5,3]]  (:198-203)
  stresses              per-atom virial, model order xx,yy,zz,xy,yz,zx                  (:212-216)
  num_edges
and the same errors (`ValueError` on bad file_type, unknown atomic number, modal misuse).
ASE itself is optional: without it the class is a plain object whose
`compute(numbers, positions, cell, pbc)` returns the same results dict.
"""
from __future__ import annotations

import os
import pathlib
import warnings
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch

from .atoms import Calculator, ManyAtomsMixin, all_changes
from .engine import HipForceEngine, build_graph
from .neighbor import neighbor_list
from .neighbor_gpu import build_graph_gpu, gpu_neighbor_supported

_OLD_MODULE_NAMES = {
    'EdgeEmbedding': 'edge_embedding',
    'reducing nn input to hidden': 'reduce_input_to_hidden',
    'reducing nn hidden to energy': 'reduce_hidden_to_energy',
    'rescale atomic energy': 'rescale_atomic_energy',
}
for _i in range(10):
    for _old, _new in (('self connection intro', 'self_connection_intro'), ('convolution', 'convolution'),
                       ('self interaction 2', 'self_interaction_2'), ('equivariant gate', 'equivariant_gate')):
        _OLD_MODULE_NAMES[f'{_i} {_old}'] = f'{_i}_{_new}'


def map_old_state_dict(state_dict):
    """Module names of checkpoints written before the 2024-04 renaming -> current names, and the
    'denumerator' spelling -> 'denominator' (map_old_model, scripts/backward_compatibility.py:44-76)."""
    out = {}
    for k, v in state_dict.items():
        head, _, follower = k.partition('.')
        follower = follower.replace('denumerator', 'denominator')
        head = _OLD_MODULE_NAMES.get(head, head)
        out[head + ('.' + follower if follower else '')] = v
    return out


def patch_old_config(cfg: dict) -> dict:
    """Defaults that configs of version <= 0.9 lack (patch_old_config, backward_compatibility.py:18-41)."""
    version = cfg.get('version')
    if not version:
        raise ValueError('No version found in config')
    major, minor = (int(t) for t in str(version).split('.')[:2])
    if major == 0 and minor <= 9:
        cf = cfg.get('cutoff_function')
        if isinstance(cf, dict) and cf.get('cutoff_function_name') == 'XPLOR':
            cf.pop('poly_cut_p_value', None)
        if 'train_denominator' not in cfg:
            cfg['train_denominator'] = cfg.pop('train_avg_num_neigh', False)
        if cfg.pop('optimize_by_reduce', None) is False:
            raise ValueError('This checkpoint(optimize_by_reduce: False) is no longer supported')
        cfg.setdefault('conv_denominator', 0.0)
        cfg.setdefault('_normalize_sph', False)
    return cfg


W3J_KEY = '{t}_convolution.convolution._compiled_main_left_right._w3j_{l1}_{l2}_{l3}'


def fix_old_convolution_signs(cfg: dict, sd: dict, strict_reference: bool = False) -> dict:
    """Second half of the reference's `sort_old_convolution` (scripts/backward_compatibility.py:119-137).

    Checkpoints with the pre-0.11 convolution (version < 0.11.0 or 0.11.0.dev0) carry the real Wigner-3j
    tensors their e3nn build compiled into the tensor product, as buffers
    `{t}_convolution.convolution._compiled_main_left_right._w3j_{l1}_{l2}_{l3}`.  Some e3nn builds stored a
    tensor with the opposite global sign of today's `o3.wigner_3j`.  The engine always contracts with
    today's tensor (its generator is pinned to it, tests/golden/w3j_cp0.npz), so for every path with
    l1, l2, l3 > 0 whose stored buffer is the negative of the generator's, the path's columns of the
    radial MLP's last layer are negated (w * (-C) == (-w) * C) -- the weight-column *permutation* half of
    `sort_old_convolution` is not needed: the column offsets follow the checkpoint's instruction order
    (model_spec.build_model_spec, `old_convolution_order`).  A buffer that is neither +C nor -C raises.

    Deliberate difference from the reference: a buffer is shared by all paths of one (l1, l2, l3)
    (O(3) models have e.g. 1o x 1o -> 1e and 1e x 1o -> 1o on `_w3j_1_1_1`); the reference negates the
    buffer IN PLACE after fixing the first such path (`stct[conv_w3j_key] *= -1` aliases `w3j_old`),
    so later paths of the same key keep their weights while their tensor has changed sign.  Here every
    path that reads a flipped buffer is fixed, which preserves the function the checkpoint was trained as.
    All released checkpoints (SO(3)-only, one path per key) are unaffected by the difference.
    When a flipped buffer IS shared by several paths a warning says so, and `strict_reference=True`
    (or SNET_STRICT_REFERENCE_W3J=1) reproduces the upstream behaviour instead: only the first path of a key is
    negated, so that this engine's numbers equal upstream's for such a checkpoint.
    Returns a state dict without the `_w3j_*` buffers."""
    from .irreps import real_wigner_3j
    from .model_spec import build_model_spec, old_convolution_order
    out = {k: v for k, v in sd.items() if '._w3j_' not in k}
    if not old_convolution_order(cfg.get('version', '0.0.0')) or len(out) == len(sd):
        return out   # current instruction order, or a checkpoint stripped of its buffers: nothing to compare
    spec = build_model_spec(cfg)   # paths in the checkpoint's own (unsorted) instruction order
    strict_reference = strict_reference or os.environ.get('SNET_STRICT_REFERENCE_W3J') == '1'
    for ls in spec.layers:
        flipped = {}
        ww_key = f'{ls.t}_convolution.weight_nn.layer{len(ls.mlp_dims) - 2}.weight'
        ww = None
        for p in ls.conv_full.paths:   # the checkpoint's column layout (the engine may have pruned unread paths)
            if not (p.l1 > 0 and p.l2 > 0 and p.l3 > 0):
                continue
            key = W3J_KEY.format(t=ls.t, l1=p.l1, l2=p.l2, l3=p.l3)
            if key not in sd:
                continue   # checkpoint stripped of buffers: nothing to compare with
            old = np.asarray(sd[key], dtype=np.float64)
            now = real_wigner_3j(p.l1, p.l2, p.l3)
            if old.shape != now.shape:
                raise ValueError(f'{key}: shape {old.shape} != {now.shape}')
            if np.allclose(old, now, rtol=1e-5, atol=1e-6):
                continue
            if not np.allclose(old, -now, rtol=1e-5, atol=1e-6):
                raise ValueError(f'{key} is neither +wigner_3j nor -wigner_3j: the checkpoint was written with an '
                                 'incompatible Clebsch-Gordan convention (e3nn < 0.4?)')
            flipped[key] = flipped.get(key, 0) + 1
            if strict_reference and flipped[key] > 1:
                continue   # upstream flipped the shared buffer in place after the first path: later paths keep their weights
            if ww is None:
                ww = np.array(out[ww_key], copy=True)
            ww[:, p.w_off:p.w_off + p.mul] *= -1.0
        if ww is not None:
            out[ww_key] = ww
        shared = sorted(k for k, c in flipped.items() if c > 1)
        if shared:
            warnings.warn(f'{shared}: a sign-flipped Wigner-3j buffer is shared by several tensor-product paths; '
                          + ('only the first path of each was negated, as sevenn/scripts/backward_compatibility.py does '
                             '(strict_reference)' if strict_reference else
                             'every such path was negated (the function the checkpoint was trained as); upstream negates only '
                             'the first -- pass strict_reference=True / SNET_STRICT_REFERENCE_W3J=1 to reproduce its numbers'))
    return out


def load_reference_checkpoint(path: str, strict_reference: bool = False):
    """(config, state_dict) from a reference checkpoint file (sevenn/checkpoint.py:286-308:
    a torch pickle holding 'config' and 'model_state_dict'), with the reference's own
    backward-compatibility steps (patch_state_dict_if_old, scripts/backward_compatibility.py:165-184):
    old config defaults, old module names, and `sort_old_convolution` -- its weight-column permutation is
    absorbed by deriving the column offsets from the checkpoint's instruction order
    (model_spec.old_convolution_order), its Wigner-3j sign fix is `fix_old_convolution_signs`."""
    cp = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(cp, dict) or 'config' not in cp or 'model_state_dict' not in cp:
        raise ValueError(f'{path} is not a SevenNet checkpoint (config + model_state_dict expected)')
    cfg = patch_old_config(dict(cp['config']))
    sd = {k: v.detach().cpu().numpy() for k, v in map_old_state_dict(cp['model_state_dict']).items()
          if hasattr(v, 'detach')}
    return cfg, fix_old_convolution_signs(cfg, sd, strict_reference)


class SevenNetCalculator(ManyAtomsMixin, Calculator):
    """Supporting properties: 'free_energy', 'energy', 'forces', 'stress', 'stresses', 'energies'."""

    implemented_properties = ['free_energy', 'energy', 'forces', 'stress', 'stresses', 'energies']

    def __init__(
        self,
        model: Union[str, pathlib.PurePath, tuple] = '7net-0',
        file_type: str = 'checkpoint',
        device: Union[torch.device, str] = 'auto',
        modal: Optional[str] = None,
        enable_cueq: Optional[bool] = False,   # accepted for signature compatibility, ignored:
        enable_flash: Optional[bool] = False,  # the tensor product always runs in libsnet_hip.so
        enable_oeq: Optional[bool] = False,
        compute_atomic_virial: bool = False,
        sevennet_config: Optional[Dict] = None,
        **kwargs,
    ) -> None:
        super().__init__(**kwargs)
        self.compute_atomic_virial = compute_atomic_virial
        if isinstance(model, pathlib.PurePath):
            model = str(model)
        allowed_file_types = ['checkpoint', 'model_instance']
        file_type = file_type.lower()
        if file_type not in allowed_file_types:
            if file_type == 'torchscript':
                raise ValueError('torchscript file_type is no longer supported. '
                                 'Use checkpoint or model_instance instead.')
            raise ValueError(f'file_type not in {allowed_file_types}')
        if isinstance(device, str):
            device = 'cuda:0' if device in ('auto', 'cuda') else device
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('the HIP force engine runs on a ROCm GPU only (device must be cuda:N)')

        if file_type == 'checkpoint' and isinstance(model, str):
            if not os.path.isfile(model):
                raise ValueError(f'checkpoint file {model!r} not found (pretrained model names need the '
                                 'reference package to download/resolve them)')
            cfg, sd = load_reference_checkpoint(model)
        elif file_type == 'model_instance' and isinstance(model, tuple) and len(model) == 2:
            cfg, sd = model  # (config dict, state_dict of arrays)
        else:
            raise ValueError('Unexpected input combinations')
        self.sevennet_config = cfg if cfg is not None else sevennet_config
        tm = cfg.get('_type_map')
        if not tm:
            raise ValueError('Model must have the type_map to be used with calculator')
        self.type_map = {int(k): int(v) for k, v in tm.items()}
        self.cutoff = float(cfg['cutoff'])
        self.modal = None
        modal_map = cfg.get('_modal_map') if cfg.get('use_modality') else None
        if modal_map:  # sevenn/calculator.py:159-170
            modal_ava = list(modal_map.keys())
            if not modal:
                raise ValueError(f'modal argument missing (avail: {modal_ava})')
            if modal not in modal_ava:
                raise ValueError(f'unknown modal {modal} (not in {modal_ava})')
            self.modal = modal
        elif modal:
            warnings.warn(f'modal={modal} is ignored as model has no modal_map')
        self.model = HipForceEngine(cfg, sd, device=str(self.device), modal=self.modal)
        self._z2type = np.full(120, -1, np.int64)  # sequential.py:80-83
        self.relax_info: Optional[Dict[str, int]] = None   # counters of the last relax_many call
        self.md_info: Optional[Dict[str, int]] = None      # counters of the last md_many call
        self.neb_info: Optional[Dict[str, int]] = None     # counters of the last neb_many call
        self.vib_info: Optional[Dict[str, int]] = None     # counters of the last vibrations_many call
        self.phonon_info: Optional[Dict[str, int]] = None  # counters of the last phonons_many call
        self.elastic_info: Optional[Dict[str, int]] = None  # counters of the last elastic_many call
        for z, t in self.type_map.items():
            self._z2type[z] = t

    def set_atoms(self, atoms) -> None:
        for z in set(atoms.get_atomic_numbers()):
            if z not in self.type_map:
                raise ValueError(f'Model do not know atomic number: {z}, (knows: {list(self.type_map.keys())})')

    def compute(self, numbers, positions, cell, pbc) -> Dict[str, Any]:
        numbers = np.asarray(numbers, np.int64)
        types = self._z2type[numbers]
        if (types < 0).any():
            bad = sorted(set(numbers[types < 0].tolist()))
            raise ValueError(f'Model do not know atomic number: {bad[0]}, (knows: {list(self.type_map.keys())})')
        cell = np.asarray(cell, np.float64).reshape(3, 3)
        # per-species row lists only where a per-species (FCTP) self-connection reads them
        ns = self.model.spec.num_species if self.model.needs_species_rows else 0
        if len(numbers) and gpu_neighbor_supported(cell, pbc, self.cutoff, np.asarray(positions, np.float64)):
            # cell list on the GPU: bulk cells, slabs / wires / molecules (open axes), cells thinner than the cutoff
            g = build_graph_gpu(types, positions, cell, self.cutoff, device=str(self.device), num_species=ns, pbc=pbc)
            n_edges = g.n_edges
        else:  # singular cells only: host list
            ei, ev, _ = neighbor_list(positions, cell, pbc, self.cutoff)
            g = build_graph(types, ei, ev, device=str(self.device), num_species=ns)
            n_edges = int(ei.shape[1])
        out = self.model.compute(g, want_atomic_virial=self.compute_atomic_virial)
        energy = float(out['energy'].cpu())
        vol = abs(float(np.linalg.det(cell)))
        vir = out['virial'].cpu().numpy()  # = -sum(r (x) g): model stress * volume, order xx,yy,zz,xy,yz,zx
        stress = -(vir / vol)[[0, 1, 2, 4, 5, 3]] if vol > 0 else np.full(6, np.nan)
        res: Dict[str, Any] = {
            'free_energy': energy, 'energy': energy,
            'energies': out['atomic_energy'].cpu().numpy().astype(np.float64),
            'forces': out['forces'].cpu().numpy().astype(np.float64),
            'stress': stress, 'num_edges': n_edges,
        }
        if self.compute_atomic_virial:
            res['stresses'] = out['atomic_virial'].cpu().numpy()
        return res

    def _types_list(self, numbers_list) -> List[np.ndarray]:
        """species indices of each system's atomic numbers; ValueError on one the model does not know"""
        types_list = []
        for numbers in numbers_list:
            numbers = np.asarray(numbers, np.int64).reshape(-1)
            types = self._z2type[np.clip(numbers, 0, len(self._z2type) - 1)]
            if ((types < 0) | (numbers < 0) | (numbers >= len(self._z2type))).any():
                bad = sorted(set(numbers[(types < 0) | (numbers < 0) | (numbers >= len(self._z2type))].tolist()))
                raise ValueError(f'Model do not know atomic number: {bad[0]}, (knows: {list(self.type_map.keys())})')
            types_list.append(types)
        return types_list

    def compute_many(self, numbers_list, positions_list, cells, pbcs) -> List[Dict[str, Any]]:
        """`compute` for B structures in ONE engine call (sevennet_amd.batch): one results dict per system, in the given
        order, with the keys, units, Voigt order and stress sign of `compute`.  cells[B,3,3], pbcs[B,3] (or one [3])."""
        from .batch import batch_results, build_batch_graph
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        types_list = self._types_list(numbers_list)
        ns = self.model.spec.num_species
        g = build_batch_graph(types_list, list(positions_list), cells, pbcs, self.cutoff, ns, device=str(self.device),
                              species_rows=self.model.needs_species_rows)
        out = self.model.compute(g, want_atomic_virial=self.compute_atomic_virial)
        return batch_results(g, out, cells, self.compute_atomic_virial)

    def relax_many(self, numbers_list, positions_list, cells, pbcs, fmax: float = 0.05, steps: int = 500, **kw) -> List[Dict[str, Any]]:
        """FIRE relaxation of B structures at once (sevennet_amd.relax.relax_batch), at fixed cells or, with relax_cell=True,
        of the cells too (ASE's UnitCellFilter rule; further kw: scalar_pressure in eV/A^3, cell_mask, hydrostatic_strain,
        constant_volume; the dicts then gain `cell` [3,3] and `status`: 'converged', 'steps' or 'cell_failed').  Positions, velocities and the
        optimizer state stay on the GPU from the first step to the last, converged systems stop moving at once and leave the
        batch when enough have finished.  One dict per system, in the given order: the keys of `compute` (evaluated at the
        returned positions) plus `positions` [n,3] fp64, `converged` (largest atomic force below fmax, eV/A) and `n_steps`.
        A system that is not converged after `steps` steps is returned with converged = False.  kw: repack_below, extra (as
        relax_batch) and the FIRE parameters (relax.FIRE_DEFAULTS).  The call's counters are kept as `self.relax_info`.
        fixed_list: per system None, a bool mask [n] or an index list of atoms, or a bool mask [n,3] of Cartesian components that
        do not move (with relax_cell whole atoms only, which keep their fractional coordinates); their `positions` come back
        with the caller's bits, `converged` refers to the free components, `forces` stay the true forces, and the dicts gain
        `fixed` [n,3] (relax_batch)."""
        from .relax import relax_batch
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        results, self.relax_info = relax_batch(self.model, self._types_list(numbers_list), list(positions_list), cells, pbcs,
                                               cutoff=self.cutoff, fmax=fmax, steps=steps,
                                               want_atomic_virial=self.compute_atomic_virial, **kw)
        return results

    def neb_many(self, numbers_list, images_list, cells, pbcs, fmax: float = 0.05, steps: int = 500, **kw) -> List[Dict[str, Any]]:
        """Nudged elastic band relaxation of B bands at once (sevennet_amd.neb.neb_batch): numbers_list[b] the atomic numbers
        [n_b] of band b, images_list[b] its images [M_b, n_b, 3] (M_b >= 3; the first and the last are the fixed endpoints,
        neb.interpolate_band makes a starting band), cells[B,3,3], pbcs[B,3] (or one [3]) per band.  The moving images, their
        velocities and the optimizer state stay on the GPU from the first step to the last: per step one batched evaluation of
        all moving images, one launch that turns forces and energies into NEB forces (improved tangent, springs along it) and
        one FIRE launch that moves all images of a band as one system, as ASE's FIRE(NEB(images)) does.  kw: k (spring constant
        in eV/A^2, one or one per band; default 0.1), climb (climbing image), fixed_list (per band a bool mask or index list of
        atoms that do not move, or None), repack_below, extra (must return energies too) and the FIRE parameters
        (relax.FIRE_DEFAULTS).  Two-stage use is a second call with the first call's positions: a plain band first, then
        climb=True.  One dict per band: `images` (M_b dicts with the keys of `compute` at the returned positions plus
        `positions`, endpoints included), `converged`, `n_steps`, `status` ('converged', 'steps' or 'failed'), `neb_fmax`,
        `imax` (index into `images`), `barrier` and `barrier_reverse` (eV).  The call's counters are kept as `self.neb_info`."""
        from .neb import neb_batch
        if len(numbers_list) != len(images_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(images_list)} bands')
        results, self.neb_info = neb_batch(self.model, self._types_list(numbers_list), list(images_list), cells, pbcs,
                                           cutoff=self.cutoff, fmax=fmax, steps=steps,
                                           want_atomic_virial=self.compute_atomic_virial, **kw)
        return results

    def vibrations_many(self, numbers_list, positions_list, masses_list, cells, pbcs, **kw) -> List[Dict[str, Any]]:
        """Harmonic analysis of B structures at once (sevennet_amd.vib.vibrations_batch): the finite-difference Hessian of each
        by central differences of forces, as ASE's Vibrations does it, with the displaced copies written, evaluated in batches
        and reduced on the GPU.  masses_list in amu (the caller's: this package has no table of atomic masses).  kw: delta
        (the displacement in A, default 0.01), nfree (2 or 4 displacements per coordinate), indices (per system None, a bool
        mask or a list of the atoms that are displaced; the others are held fixed), max_atoms_per_call (a cap on the atoms of
        one batched evaluation) and extra / make_extra (as vibrations_batch).  One dict per system, in the given order: the
        keys of `compute` for the undisplaced structure (is it a stationary point?; its per-atom energies are
        `atomic_energies` here) plus `indices`, `hessian` [3m,3m] (eV/A^2), `asymmetry`, `eigenvalues` (of the mass-weighted Hessian, ascending), `modes` [3m,m,3], `energies` (h nu, eV) and `frequencies`
        (cm^-1) -- both signed: an imaginary mode is a negative number, so a minimum has none below zero and a first-order
        saddle, the top of a climbing-image band of `neb_many`, exactly one -- `zpe` (eV) and `status` ('ok' or 'failed').
        vib.harmonic_prefactor turns the `energies` of a minimum and of a saddle into the prefactor of the hop.  The call's
        counters are kept as `self.vib_info`."""
        from .vib import vibrations_batch
        if not len(numbers_list) == len(positions_list) == len(masses_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays, {len(positions_list)} position arrays and '
                             f'{len(masses_list)} mass arrays')
        results, self.vib_info = vibrations_batch(self.model, self._types_list(numbers_list), list(positions_list), list(masses_list),
                                                  cells, pbcs, cutoff=self.cutoff, want_atomic_virial=self.compute_atomic_virial, **kw)
        return results

    def phonons_many(self, numbers_list, positions_list, masses_list, cells, pbcs, supercells, *, qpoints=None, mesh=None,
                     temperatures=None, delta: float = 0.01, nfree: int = 2, acoustic: bool = True, symprec: float = 1e-5,
                     want_modes: bool = False, dos_bins=200, max_atoms_per_call: int = 32768, **kw) -> List[Dict[str, Any]]:
        """Supercell phonons of B crystals at once (sevennet_amd.phonon.phonons_batch).  numbers_list / positions_list / masses_list
        (amu) / cells / pbcs describe the PRIMITIVE cells (fully periodic), supercells the repeats (n1,n2,n3): one triple or one per
        system.  Only the home-cell atoms are displaced (nfree 3 m supercells per system, packed into batched evaluations of at
        most max_atoms_per_call atoms); the force constants against the whole supercell, the acoustic sum rule (acoustic), the
        nearest-image rule (symprec, A: equally near images share the weight) and the dynamical matrices D(q) are computed on the
        GPU.  qpoints: fractional q-points ([n_q,3], or one array per system; phonon.band_path makes a path); mesh: a
        Gamma-centred mesh for `dos` and, with temperatures (K), `thermo`; at least one of the two.  Further kw: e_min,
        max_q_per_call, extra / make_extra (as phonons_batch).  One dict per system, in the given order: the keys of `compute` for
        the undisplaced supercell (per-atom energies as `atomic_energies`) plus `supercell`, `supercell_positions`,
        `supercell_cell`, `force_constants` [m,N,3,3], `asr_defect`, `qpoints`, `eigenvalues`, `energies` (h nu in eV) and
        `frequencies` (cm^-1) [n_q,3m] -- both signed: an imaginary mode is a negative number --, `hermiticity` [n_q], `modes`
        [n_q,3m,m,3] (want_modes; the phase of D(q) is taken with the full vector between the atoms, and the modes are in that
        convention), with mesh `mesh`, `dos_energies`, `dos`, `thermo`, and `status` ('ok' or 'failed').  The call's counters
        are kept as `self.phonon_info`."""
        from .phonon import phonons_batch
        if not len(numbers_list) == len(positions_list) == len(masses_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays, {len(positions_list)} position arrays and '
                             f'{len(masses_list)} mass arrays')
        results, self.phonon_info = phonons_batch(self.model, self._types_list(numbers_list), list(positions_list), list(masses_list),
                                                  cells, pbcs, supercells, cutoff=self.cutoff, qpoints=qpoints, mesh=mesh,
                                                  temperatures=temperatures, delta=delta, nfree=nfree, acoustic=acoustic,
                                                  symprec=symprec, want_modes=want_modes, dos_bins=dos_bins,
                                                  max_atoms_per_call=max_atoms_per_call,
                                                  want_atomic_virial=self.compute_atomic_virial, **kw)
        return results

    def elastic_many(self, numbers_list, positions_list, cells, pbcs, *, delta: float = 0.005, nfree: int = 2,
                     relax_ions: bool = False, ion_delta: float = 0.01, max_atoms_per_call: int = 32768, **kw) -> List[Dict[str, Any]]:
        """Second-order elastic tensors of B crystals at once (sevennet_amd.elastic.elastic_batch): central differences of the
        stress over 6 nfree homogeneously strained copies per system (strain step delta, a shear step being the engineering
        strain; nfree 2 or 4), written, evaluated in batches of at most max_atoms_per_call atoms and reduced on the GPU.  Every
        system must be periodic along all three axes.  relax_ions: also let the ions follow the strain, through the Gamma
        Hessian (vibrations_many's kernels, displacement ion_delta in A) and the internal-strain tensor.  Further kw: extra /
        make_extra (as elastic_batch).  One dict per system, in the given order: the keys of `compute` for the unstrained
        structure plus `stress_strain` [6,6] (raw d sigma_i / d epsilon_j, eV/A^3, Voigt order xx, yy, zz, yz, xz, xy),
        `elastic_tensor` [6,6] (its symmetric part: the elastic tensor where the unstrained `stress` is about zero),
        `asymmetry`, `internal_strain` [n,3,6], `fmax`, `compliance`, `bulk_modulus` / `shear_modulus` (`voigt`, `reuss`, `hill`),
        `youngs_modulus`, `poisson_ratio`, `stable` and `status` ('ok', 'failed' or 'singular'); with relax_ions `elastic_tensor`
        is the relaxed-ion one, beside `elastic_tensor_clamped`, `hessian` and `ion_eigenvalues`.  elastic.GPA converts to GPa.
        The call's counters are kept as `self.elastic_info`."""
        from .elastic import elastic_batch
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        results, self.elastic_info = elastic_batch(self.model, self._types_list(numbers_list), list(positions_list), cells, pbcs,
                                                   cutoff=self.cutoff, delta=delta, nfree=nfree, relax_ions=relax_ions,
                                                   ion_delta=ion_delta, max_atoms_per_call=max_atoms_per_call,
                                                   want_atomic_virial=self.compute_atomic_virial, **kw)
        return results

    def md_many(self, numbers_list, positions_list, masses_list, cells, pbcs, dt: float, steps: int, **kw) -> List[Dict[str, Any]]:
        """`steps` steps of `dt` fs of NVE or Langevin MD for B structures at once (sevennet_amd.md.md_batch): positions,
        velocities, energy logs and trajectory frames stay on the GPU from the first step to the last and come to the host
        once.  masses_list in amu (the caller's: this package has no table of atomic masses).  kw: temperature (K, scalar
        or per system), friction (1/fs; 0 = NVE), velocities (A/fs; None: drawn at `temperature`), seed, log_every,
        traj_every, remove_com, system_ids, extra (as md_batch).  One dict per system, in the given order: the keys of `compute` (the last
        engine call, at the returned positions) plus `positions`, `velocities`, `e_pot`, `e_kin`, `temperature` and, with
        traj_every > 0, `trajectory`.  The call's counters are kept as `self.md_info`.
        With pressure= (eV/A^3, scalar or per system) the run is isotropic NPT by stochastic cell rescaling, the cells moving on
        the GPU too: further kw compressibility (A^3/eV, required), barostat_time (fs, default 1000) and max_log_volume_step
        (default 0.1); every system fully periodic with at most batch.BATCH_MAX_ATOMS atoms.  The dicts then gain `cell` [3,3]
        (the keys of `compute` are those at the returned positions AND cell), `volume` and `pressure` over the logged steps and
        `status`: 'ok' or 'cell_failed' (md_batch).
        fixed_list: per system None, a bool mask [n] or an index list of atoms, or a bool mask [n,3] of Cartesian components that
        do not move: no kick, no drift, no noise, velocity 0 (held components of `velocities` are set to 0), `temperature`
        over the remaining degrees of freedom; the dicts gain `fixed` [n,3].  Not together with pressure= (md_batch).
        observe: an observe.Observe -- RDF pair counts, mean-square displacement and velocity autocorrelation accumulated on the
        GPU every `every` steps, nothing read back before the end; the dicts gain `observables` (observe.attach_observables), its
        `kinds` as atomic numbers.  Not together with pressure= (md_batch)."""
        from .md import md_batch
        if not len(numbers_list) == len(positions_list) == len(masses_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays, {len(positions_list)} position arrays and '
                             f'{len(masses_list)} mass arrays')
        results, self.md_info = md_batch(self.model, self._types_list(numbers_list), list(positions_list), list(masses_list), cells,
                                         pbcs, cutoff=self.cutoff, dt=dt, steps=steps,
                                         want_atomic_virial=self.compute_atomic_virial, **kw)
        if kw.get('observe') is not None:   # kinds: the model's species indices -> atomic numbers
            z_of = {t: z for z, t in self.type_map.items()}
            for r in results:
                kinds = r['observables']['kinds']
                if kinds is not None:
                    r['observables']['kinds'] = np.array([z_of[int(t)] for t in kinds], np.int64)
        return results

    def calculate(self, atoms=None, properties=None, system_changes=all_changes):
        Calculator.calculate(self, atoms, properties, system_changes)
        if atoms is None:
            raise ValueError('No atoms to evaluate')
        self.results = self.compute(atoms.get_atomic_numbers(), atoms.get_positions(),
                                    np.array(atoms.get_cell()), atoms.get_pbc())
