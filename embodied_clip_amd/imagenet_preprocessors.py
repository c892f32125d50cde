"""Drop-in ``ResNetPreprocessor``: AllenAct's ImageNet-ResNet feature preprocessor on the HIP trunks.

Same constructor keywords, observation space and ``process`` / ``to`` behaviour as [U]
``allenact/embodiedai/preprocessors/resnet.py`` ``ResNetPreprocessor`` (the class the ImageNet baselines
``objectnav_robothor_rgb_resnet18gru_ddppo`` / ``objectnav_robothor_rgb_resnet50gru_ddppo`` feed into
``ResnetTensorObjectNavActorCritic``: readme_files/imagenet_vs_objectnav.md, baselines_robothor_objectnav.md:47).
The arithmetic behind ``process`` is the hand-written gfx950 path: ``ImageNetBasicTrunk`` (ResNet-18 / 34) or
``ImageNetRN50Trunk`` (ResNet-50 / 101 / 152) instead of ``torchvision_resnet_model(pretrained=True)``.

Weights: this class never downloads.  The torchvision ``state_dict`` comes from ``state_dict=`` / ``weights_path=``,
then ``$EC_TORCHVISION_WEIGHTS_DIR/<name>*.pth``, then torch's hub cache (``<torch.hub.get_dir()>/checkpoints/<name>-*.pth``,
where ``pretrained=True`` leaves it).
"""
from __future__ import annotations

import glob
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import spaces
from .allenact_compat import Preprocessor
from .encoder import IMAGENET_RGB_MEANS, IMAGENET_RGB_STDS

# name -> (block layers, output channels, basic block)
ARCHS: Dict[str, Tuple[Tuple[int, int, int, int], int, bool]] = {
    "resnet18": ((2, 2, 2, 2), 512, True),
    "resnet34": ((3, 4, 6, 3), 512, True),
    "resnet50": ((3, 4, 6, 3), 2048, False),
    "resnet101": ((3, 4, 23, 3), 2048, False),
    "resnet152": ((3, 8, 36, 3), 2048, False),
}


def resnet_name(model: Any) -> str:
    """``torchvision.models.resnet18`` (or any callable / string with that name) -> ``"resnet18"``; unknown names raise."""
    name = model if isinstance(model, str) else getattr(model, "__name__", None)
    if not isinstance(name, str) or name not in ARCHS:
        raise ValueError(f"ResNetPreprocessor: unsupported torchvision_resnet_model {model!r}; expected one of {sorted(ARCHS)}")
    return name


def find_weights(name: str, state_dict=None, weights_path: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The torchvision ``state_dict`` of ``name`` from, in order, ``state_dict`` / ``weights_path``,
    ``$EC_TORCHVISION_WEIGHTS_DIR`` and torch's hub cache.  Nothing is downloaded."""
    if state_dict is not None:
        return dict(state_dict)
    tried = []
    cands: List[str] = []
    if weights_path is not None:
        cands.append(weights_path)
        tried.append(f"weights_path={weights_path!r}")
    env = os.environ.get("EC_TORCHVISION_WEIGHTS_DIR")
    if env:
        cands += sorted(glob.glob(os.path.join(env, f"{name}.pth")) + glob.glob(os.path.join(env, f"{name}-*.pth")))
    tried.append(f"$EC_TORCHVISION_WEIGHTS_DIR/{name}*.pth ({env or 'unset'})")
    hub = os.path.join(torch.hub.get_dir(), "checkpoints")
    cands += sorted(glob.glob(os.path.join(hub, f"{name}-*.pth")))
    tried.append(f"torch hub cache {hub}/{name}-*.pth")
    for c in cands:
        if os.path.exists(c):
            sd = torch.load(c, map_location="cpu", weights_only=True)
            return dict(sd.get("state_dict", sd)) if isinstance(sd, dict) else dict(sd)
    raise FileNotFoundError(f"No weights for torchvision {name}: pass state_dict= (or weights_path=), or provide one of: "
                            + "; ".join(tried) + ".  (ResNetPreprocessor never downloads.)")


class ResNetPreprocessor(Preprocessor):
    """[U] ``ResNetPreprocessor(input_height, input_width, output_height, output_width, output_dims, pool,
    torchvision_resnet_model=models.resnet18, device=None, device_ids=None, input_uuids=[...], output_uuid=...)``.

    ``process(obs)``: ``obs[input_uuids[0]]`` fp32 NHWC [N,H,W,3] already normalised by the sensor (ImageNet mean / std),
    or raw uint8 [N,H,W,3] (normalisation fused into the stem); a one-channel (depth) frame is repeated to 3 channels, as
    upstream does.  Returns fp32 NCHW [N,C,H/32,W/32] (``pool=False``) or [N,C] (``pool=True``) on ``device``."""

    def __init__(self, input_height: int, input_width: int, output_height: int, output_width: int, output_dims: int,
                 pool: bool, torchvision_resnet_model: Any = "resnet18", device: Optional[torch.device] = None,
                 device_ids: Optional[List[torch.device]] = None, state_dict=None, weights_path: Optional[str] = None,
                 chunk: int = 0, **kwargs: Any):
        self.arch = resnet_name(torchvision_resnet_model)
        layers, channels, self._basic = ARCHS[self.arch]
        if input_height != input_width or input_height % 32 != 0:
            raise ValueError(f"ResNetPreprocessor: square frames with a side divisible by 32 expected, got {input_height}x{input_width}")
        S = input_height // 32
        if (output_dims, output_height, output_width) != (channels, S, S):
            raise ValueError(f"ResNetPreprocessor: {self.arch} on {input_height}x{input_width} frames gives "
                             f"({channels}, {S}, {S}), not (output_dims, output_height, output_width) = "
                             f"({output_dims}, {output_height}, {output_width})")
        self.input_height, self.input_width = input_height, input_width
        self.output_height, self.output_width, self.output_dims = output_height, output_width, output_dims
        self.pool = pool
        self._layers = layers
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.device_ids = device_ids or []
        self._state_dict, self._weights_path, self._chunk = state_dict, weights_path, chunk
        self._model = None
        input_uuids = kwargs.get("input_uuids")
        output_uuid = kwargs.get("output_uuid")
        assert input_uuids is not None and len(input_uuids) == 1, "ResNetPreprocessor takes exactly one input uuid"
        assert output_uuid is not None, "ResNetPreprocessor needs output_uuid"
        shape = (output_dims,) if pool else (output_dims, output_height, output_width)
        super().__init__(input_uuids=list(input_uuids), output_uuid=output_uuid,
                         observation_space=spaces.Box(low=-np.inf, high=np.inf, shape=shape, dtype=np.float32))

    @property
    def resnet(self):
        if self._model is None:   # lazy, like upstream
            from .encoder import ImageNetBasicTrunk, ImageNetRN50Trunk, _layers
            sd = {k: v for k, v in find_weights(self.arch, self._state_dict, self._weights_path).items() if not k.startswith("fc.")}
            if tuple(_layers(sd)) != self._layers or (any(".conv3." in k for k in sd) == self._basic):
                raise ValueError(f"ResNetPreprocessor: the weights are not a torchvision {self.arch} "
                                 f"(blocks per layer {_layers(sd)}, expected {self._layers})")
            cls = ImageNetBasicTrunk if self._basic else ImageNetRN50Trunk
            self._model = cls(sd, device=self.device, input_resolution=self.input_height, chunk=self._chunk)
        return self._model

    def to(self, device: torch.device) -> "ResNetPreprocessor":
        self.device = torch.device(device)
        self._model = None   # rebuilt lazily on the new device
        return self

    def process(self, obs: Dict[str, Any], *args: Any, **kwargs: Any) -> torch.Tensor:
        x = obs[self.input_uuids[0]]
        if x.shape[-1] == 1:      # depth input: repeated to 3 channels, as upstream does
            x = x.expand(*x.shape[:-1], 3)
        trunk = self.resnet
        if x.dtype == torch.uint8:   # raw frames: /255 and the ImageNet mean / std are fused into the stem kernel
            feat = trunk.forward_u8(x.to(self.device).contiguous(), mean=IMAGENET_RGB_MEANS, std=IMAGENET_RGB_STDS)
        else:
            feat = trunk.forward(x.to(self.device, dtype=torch.float32).contiguous())
        return trunk.spatial_mean(feat) if self.pool else trunk.to_nchw_f32(feat)

    def process_bf16_nhwc(self, rgb: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Device fp32 NHWC frame -> bf16 NHWC [N,S,S,C] written straight into ``out`` (e.g. a rollout feature slice)."""
        return self.resnet.forward(rgb, out)
