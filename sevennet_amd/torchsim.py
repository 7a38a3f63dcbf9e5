"""TorchSim-style batched model interface over the HIP force engine.

Counterpart of the reference's `sevenn.torchsim.SevenNetModel` (sevenn/torchsim.py:56-292): the same constructor
arguments and `forward(state)` contract -- a batch of systems in, `energy[B]`, `forces[N,3]` and `stress[B,3,3]` out, with
the reference's sign and Voigt mapping (`-voigt_6_to_full_3x3(stress[..., [0, 1, 2, 4, 5, 3]])`).  The state is read
duck-typed (`positions`, `row_vector_cell`, `pbc`, `atomic_numbers`, `system_idx`), so torch_sim itself is not needed;
device tensors stay on the device.  One evaluation is ONE engine call over the batch graph of sevennet_amd.batch.
"""
from __future__ import annotations

from pathlib import Path
from typing import Callable, Dict, Optional, Union

import numpy as np
import torch

from .batch import build_batch_graph, voigt_to_3x3
from .calculator import SevenNetCalculator


class SevenNetModel(torch.nn.Module):
    """Computes energies, forces and stresses of a batch of systems with a SevenNet model.

    model: a checkpoint path, or a (config, state_dict) pair (the calculator's `model_instance`).  neighbor_list_fn and the
    cuEquivariance / flashTP / OpenEquivariance switches are accepted for signature compatibility and ignored: the graph is
    built by the batched HIP neighbor list and the tensor product always runs in libsnet_hip.so."""

    def __init__(self, model: Union[str, Path, tuple], *, modal: Optional[str] = None, neighbor_list_fn: Optional[Callable] = None,
                 enable_cueq: bool = False, enable_flash: bool = False, enable_oeq: bool = False,
                 compute_atomic_virial: bool = False, device: Union[torch.device, str] = 'auto',
                 dtype: torch.dtype = torch.float32) -> None:
        if compute_atomic_virial:
            raise NotImplementedError('compute_atomic_virial is not supported for SevenNet TorchSim interface.')
        if dtype is not torch.float32:
            raise ValueError(f'SevenNet currently only supports {torch.float32}, but received different dtype: {dtype}')
        super().__init__()
        file_type = 'model_instance' if isinstance(model, tuple) else 'checkpoint'
        self._calc = SevenNetCalculator(model, file_type=file_type, device=device, modal=modal)
        self._device = self._calc.device
        self._dtype = dtype
        self._memory_scales_with = 'n_atoms_x_density'
        self._compute_stress = True
        self._compute_forces = True
        self.neighbor_list_fn = neighbor_list_fn
        self.modal = self._calc.modal
        self.type_map = dict(self._calc.type_map)
        self.cutoff = torch.tensor(self._calc.cutoff)
        self.implemented_properties = ['energy', 'forces', 'stress']
        self._z2type = torch.as_tensor(self._calc._z2type).to(self._device)

    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def dtype(self) -> torch.dtype:
        return self._dtype

    def forward(self, state, **kwargs) -> Dict[str, torch.Tensor]:
        """energy [B], forces [N,3] and stress [B,3,3] (eV, eV/A, eV/A^3) of the systems of `state`; atoms of one system
        must be contiguous (system_idx non-decreasing), as torch_sim's SimState keeps them"""
        dev = self._device
        pos = torch.as_tensor(state.positions).to(dev, torch.float64)
        cell = torch.as_tensor(state.row_vector_cell).to(dev, torch.float64).reshape(-1, 3, 3)
        z = torch.as_tensor(state.atomic_numbers).to(dev, torch.int64).reshape(-1)
        sys_idx = torch.as_tensor(state.system_idx).to(dev, torch.int64).reshape(-1)
        B = int(cell.shape[0])
        n_atoms = torch.bincount(sys_idx, minlength=B)
        if n_atoms.numel() != B or (sys_idx.numel() > 1 and bool((sys_idx[1:] < sys_idx[:-1]).any())):
            raise ValueError('system_idx must number the systems 0 .. B-1 with the atoms of each system contiguous')
        pbc = np.asarray(state.pbc.detach().cpu().numpy() if isinstance(state.pbc, torch.Tensor) else state.pbc, bool)
        pbc = np.broadcast_to(pbc.reshape(-1, 3) if pbc.size >= 3 else np.full((1, 3), bool(pbc)), (B, 3))
        types = torch.where((z >= 0) & (z < self._z2type.numel()), self._z2type[z.clamp(0, self._z2type.numel() - 1)], -1)
        eng = self._calc.model
        g = build_batch_graph(types, pos, cell, pbc, self._calc.cutoff, eng.spec.num_species, n_atoms=n_atoms.cpu().numpy(),
                              device=str(dev), species_rows=eng.needs_species_rows)
        out = eng.compute(g)
        vol = torch.det(cell)   # signed, as the reference (sevenn/torchsim.py:245)
        model_stress = out['virial_per_system'] / vol.unsqueeze(-1)   # force_output.py:226-228 with its sign folded in
        stress = -voigt_to_3x3(model_stress[..., [0, 1, 2, 4, 5, 3]])
        return {'energy': out['energy_per_system'].to(self._dtype).detach(), 'forces': out['forces'].to(self._dtype).detach(),
                'stress': stress.to(self._dtype).detach()}
