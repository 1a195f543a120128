"""Host-side mirror of modules/utils/detection.py:24-130 -- the sequence bookkeeping of the reference's training step
(modules/detection.py:113-177): `BackboneFeatureSelector` (label-sparse gather of the backbone features over the timesteps
of a sequence) and `RNNStates` (recurrent states kept per data-loader worker, detached between steps, reset per sample).

Same class and method names as the reference.  The data movement runs in libsast_hip.so: the gather of the selected samples
of all timesteps is ONE launch per feature map (`sast_gather_samples`, backward `sast_gather_samples_bwd`), the per-sample
state reset is `sast_zero_samples`.  Feature maps may be logical NCHW tensors in channels-last memory (what the modules of
this package return) or NHWC buffers; a sample is a contiguous chunk either way.

`DeviceFeatureSelector` and `RNNStates.reset_on_device` are the same two operations with the selection in DEVICE memory
(`functional.SelectionTable`, a flags tensor): nothing of the label pattern or of the sequence starts is a kernel argument, so a
captured training step follows them from replay to replay (`sast_gather_samples_dev`, `sast_zero_samples_dev`).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Union

import torch

from .. import functional as SF


class BackboneFeatureSelector:
    """modules/utils/detection.py:24-47"""

    def __init__(self):
        self.features = None
        self.reset()

    def reset(self):
        self.features: Dict[int, List] = dict()

    def add_backbone_features(self, backbone_features: Dict[int, torch.Tensor], selected_indices: Optional[List[int]] = None) -> None:
        if selected_indices is not None:
            assert len(selected_indices) > 0
        for k, v in backbone_features.items():
            idx = list(range(v.shape[0])) if selected_indices is None else [int(i) % v.shape[0] for i in selected_indices]
            self.features.setdefault(k, []).append((v, idx))

    def get_batched_backbone_features(self) -> Optional[Dict[int, torch.Tensor]]:
        if len(self.features) == 0:
            return None
        return {k: SF.gather_samples([v for v, _ in items], [i for _, i in items]) for k, items in self.features.items()}


class DeviceFeatureSelector:
    """BackboneFeatureSelector with the selection in device memory (`SF.SelectionTable`): the feature maps of EVERY timestep are added,
    in order, and the labelled (timestep, sample) pairs are read from the table when the gather kernel runs -- one launch per feature
    map, and a captured step follows the label pattern of each replay.  The batch of the result is the table's n_out."""

    def __init__(self, sel: "SF.SelectionTable"):
        self.sel = sel
        self.features = None
        self.reset()

    def reset(self):
        self.features: Dict[int, List[torch.Tensor]] = dict()

    def add_backbone_features(self, backbone_features: Dict[int, torch.Tensor]) -> None:
        for k, v in backbone_features.items():
            self.features.setdefault(k, []).append(v)

    def get_batched_backbone_features(self) -> Optional[Dict[int, torch.Tensor]]:
        if len(self.features) == 0:
            return None
        for k, xs in self.features.items():
            if len(xs) != self.sel.T:
                raise RuntimeError(f"sast_amd: DeviceFeatureSelector holds {len(xs)} timesteps of feature map {k}, the selection table is for {self.sel.T}")
        return {k: SF.gather_samples_dev(xs, self.sel) for k, xs in self.features.items()}


def _map_leaves(tree, fn):
    """fn applied to every tensor of a nested list / tuple / dict of tensors; the containers are rebuilt with their own types"""
    if torch.is_tensor(tree):
        return fn(tree)
    if isinstance(tree, dict):
        return {key: _map_leaves(val, fn) for key, val in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_map_leaves(val, fn) for val in tree)
    raise NotImplementedError(f"RNNStates: unsupported state container {type(tree).__name__}")


def _zero_selected(which):
    if which is not None and len(which) == 0:
        raise AssertionError("RNNStates.reset: an empty selection (pass None to reset every sample)")

    def zero(t: torch.Tensor) -> torch.Tensor:
        if t.requires_grad:
            raise AssertionError("RNNStates.reset: saved states are detached; got a tensor that requires grad")
        return SF.zero_samples(t, which)       # in place, one launch per state tensor (sast_zero_samples)
    return zero


class RNNStates:
    """Recurrent states per data-loader worker (the role of modules/utils/detection.py:76-130; same method names so that
    modules/detection.py:141-177 can drive it): a table worker_id -> nested [(h, c) per stage], stored detached, selected
    samples zeroed at sequence starts.  The tree walk is `_map_leaves`; the zeroing runs on the device."""

    def __init__(self):
        self.states = {}

    @classmethod
    def recursive_detach(cls, inp):
        return _map_leaves(inp, torch.Tensor.detach)

    @classmethod
    def recursive_reset(cls, inp, indices_or_bool_tensor: Optional[Union[List[int], torch.Tensor]] = None):
        return _map_leaves(inp, _zero_selected(indices_or_bool_tensor))

    def save_states_and_detach(self, worker_id: int, states) -> None:
        self.states[worker_id] = self.recursive_detach(states)

    def get_states(self, worker_id: int):
        return self.states.get(worker_id)

    def reset(self, worker_id: int, indices_or_bool_tensor: Optional[Union[List[int], torch.Tensor]] = None):
        held = self.states.get(worker_id)
        if held is not None:
            self.states[worker_id] = self.recursive_reset(held, indices_or_bool_tensor)

    def reset_on_device(self, worker_id: int, flags: torch.Tensor) -> None:
        """`reset` with the selection as a device tensor (uint8 / bool [B], != 0: the sample starts a new sequence): every held state
        tensor in ONE launch (`sast_zero_samples_dev`), no copy of the flags to the host -- capturable, and a replay follows its flags"""
        held = self.states.get(worker_id)
        if held is None:
            return
        leaves = []

        def collect(t: torch.Tensor) -> torch.Tensor:
            if t.requires_grad:
                raise AssertionError("RNNStates.reset_on_device: saved states are detached; got a tensor that requires grad")
            leaves.append(t)
            return t
        _map_leaves(held, collect)
        SF.zero_samples_dev(leaves, flags)
