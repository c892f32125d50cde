"""Test helper: a restatement of torchvision's BasicBlock ResNet (resnet18 / resnet34) trunk,
``Sequential(*list(resnet18().children())[:-2])``, in fp32 with an optional bf16-rounding emulation at the rounding
points of the HIP plan (ec_tvresnet_basic_create):

  * the frame, the folded weights and the stem output (after the max-pool) are rounded;
  * conv1 + bn1 + relu is rounded;
  * conv2 + bn2 + identity + relu is rounded ONCE; in a transition block the 1x1 stride-2 downsample conv + bn runs in
    the same GEMM (K-concatenated, summed bias), so its output is not rounded on its own.

Pinned to HuggingFace ``ResNetModel(layer_type="basic")`` by tests/test_tvresnet_basic.py."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle.clip_resnet import _conv_bn, _layer_cfg, _r


def basic_block(x, sd, p, stride, emulate=False, fold=True):
    """torchvision ``BasicBlock.forward``: relu(bn2(conv2(relu(bn1(conv1(x))))) + downsample(x))."""
    out = _r(F.relu(_conv_bn(x, sd, p + ".conv1", p + ".bn1", stride=stride, padding=1, emulate=emulate, fold=fold)), emulate)
    out = _conv_bn(out, sd, p + ".conv2", p + ".bn2", padding=1, emulate=emulate, fold=fold)
    if (p + ".downsample.0.weight") in sd:
        idt = _conv_bn(x, sd, p + ".downsample.0", p + ".downsample.1", stride=stride, emulate=emulate, fold=fold)
    else:
        idt = x
    return _r(F.relu(out + idt), emulate)


def basic_trunk(x_nchw: torch.Tensor, sd: Dict[str, torch.Tensor], emulate_bf16: bool = False, fold: bool = True):
    """fp32 [B,3,R,R] ImageNet-normalised -> fp32 [B,512,R/32,R/32]."""
    e = emulate_bf16
    with torch.no_grad():
        x = _r(x_nchw.float(), e)
        x = F.relu(_conv_bn(x, sd, "conv1", "bn1", stride=2, padding=3, emulate=e, fold=fold))
        x = _r(F.max_pool2d(x, kernel_size=3, stride=2, padding=1), e)
        for li, nblocks in enumerate(_layer_cfg(sd), start=1):
            for b in range(nblocks):
                x = basic_block(x, sd, f"layer{li}.{b}", 2 if (b == 0 and li > 1) else 1, emulate=e, fold=fold)
        return x
