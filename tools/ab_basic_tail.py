"""A/B of the BasicBlock transition tail (ResNet-18 / 34, first block of layers 2-4), called directly through ctypes:

  A  ec_basic_tail_s2_bf16: conv2 3x3 + 1x1 stride-2 downsample + summed bias + ReLU as ONE K-concatenated GEMM
  B  the two-launch composition: ec_conv_bf16_s2 (1x1 stride-2 downsample, no activation) -> ec_conv_bf16 (3x3 conv2
     with that output as the residual, ReLU)

at 32 / 128 / 256 frames.  Median of `--reps` HIP-event-timed launches after warm-up; A and B alternate within each
repetition.  Also prints rel-L2(A, B).

    python tools/ab_basic_tail.py --reps 50
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from embodied_clip_amd import encoder as enc  # noqa: E402

SHAPES = [(28, 128, 64), (14, 256, 128), (7, 512, 256)]   # (Ho, planes, inplanes): layer2.0, layer3.0, layer4.0


def _time(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[32, 128, 256])
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"{'frames':>6} {'shape':>22} {'fused_us':>9} {'two_launch_us':>13} {'fused/two':>9} {'rel_l2':>8}")
    for B in a.frames:
        for Ho, planes, inplanes in SHAPES:
            g = torch.Generator().manual_seed(B + planes)
            c1 = torch.randn(B, Ho, Ho, planes, generator=g).relu().to(torch.bfloat16).to(dev)
            x = torch.randn(B, 2 * Ho, 2 * Ho, inplanes, generator=g).relu().to(torch.bfloat16).to(dev)
            w2 = (torch.randn(planes, 9 * planes, generator=g) * (9 * planes) ** -0.5).to(torch.bfloat16).to(dev)
            wd = (torch.randn(planes, inplanes, generator=g) * inplanes ** -0.5).to(torch.bfloat16).to(dev)
            b2, bd = (torch.randn(planes, generator=g) * 0.1).to(dev), (torch.randn(planes, generator=g) * 0.1).to(dev)
            w_cat, b_cat = torch.cat([w2, wd], 1).contiguous(), (b2 + bd).contiguous()
            out_a = torch.empty(B, Ho, Ho, planes, dtype=torch.bfloat16, device=dev)
            out_b = torch.empty_like(out_a)
            ds = torch.empty_like(out_a)
            fa = lambda: enc.basic_tail_s2_bf16(c1, x, w_cat, b_cat, out=out_a)
            fb = lambda: (enc.conv_bf16_s2(x, wd, bd, ksize=1, act=0, out=ds),
                          enc.conv_bf16(c1, w2, b2, res=ds, ksize=3, act=1, out=out_b))
            for _ in range(5):
                fa(); fb()
            ta, tb = [], []
            for _ in range(a.reps):
                ta += _time(fa, 1)
                tb += _time(fb, 1)
            ma, mb = statistics.median(ta), statistics.median(tb)
            rel = ((out_a.float() - out_b.float()).norm() / out_b.float().norm()).item()
            shape = f"{inplanes}->{planes}@{2 * Ho}->{Ho}"
            print(f"{B:>6} {shape:>22} {ma:>9.1f} {mb:>13.1f} {ma / mb:>9.3f} {rel:>8.1e}", flush=True)


if __name__ == "__main__":
    main()
