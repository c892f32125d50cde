"""Run as a subprocess by tests/test_gpu_vit_stages.py (the library reads EC_VIT_WIDE / EC_VIT_BM192 once per process): for every
case of _vit_stage_ref.gemm_cases(setting) a producer -> consumer chain through ec_gemm_bf16_ln -- a plain GEMM with residual
(in place, as the towers run it) that also emits the rows' LayerNorm records, then the LayerNorm-folded GEMM that reads them --
and the same consumer fed by ec_row_stats_bf16 records (np = 1).  Prints, per case, the worst error / bound ratios as JSON."""
import ctypes
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _guard import SENT16 as SENTINEL  # noqa: E402

PAD = 8                    # rows behind every output that must keep the sentinel


def main():
    import _vit_stage_ref as R
    from embodied_clip_amd import _lib
    setting = sys.argv[1]
    assert all(os.environ.get(k) == v for k, v in R.GEMM_SETTINGS[setting].items())
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = _lib.stream_ptr()
    K0 = 64
    results = []
    folds = {}
    for case in R.gemm_cases(setting):
        M, D, N, act, stream = case["M"], case["D"], case["N"], case["act"], case["stream"]
        res = R.residual_stream(stream, M, D)
        g = torch.Generator().manual_seed(1 + M + D)
        A = (0.25 * torch.randn(M, K0, generator=g)).to(torch.bfloat16)
        Wo = (torch.randn(D, K0, generator=g) * K0 ** -0.5).to(torch.bfloat16)
        bo = 0.1 * torch.randn(D, generator=g)
        # ---- producer: x = A Wo^T + bo + x, and the records of the stored rows
        x = torch.full((M + PAD, D), 0, dtype=torch.int16, device=dev)
        x.fill_(SENTINEL)
        x[:M] = res.view(torch.int16).to(dev)
        stats = torch.full((M + PAD, 8, 4), -7.0, dtype=torch.float32, device=dev)
        np_out = ctypes.c_int(-1)
        dA, dWo, dbo = A.to(dev), Wo.to(dev), bo.to(dev)
        _lib.check(lib.ec_gemm_bf16_ln(dA.data_ptr(), dWo.data_ptr(), dbo.data_ptr(), x.data_ptr(), x.data_ptr(), M, D, K0, R.ACT_NONE,
                                       None, None, 0, stats.data_ptr(), ctypes.byref(np_out), st), "producer")
        torch.cuda.synchronize()
        npr = np_out.value
        xs = x.cpu()
        pad_ok = bool((xs[M:] == SENTINEL).all())
        xb = xs[:M].view(torch.bfloat16)
        pref = A.double() @ Wo.double().T + bo.double()[None, :] + res.double()
        pbound = R.UB * pref.abs() + (K0 + 2) * R.U * (A.double().abs() @ Wo.double().abs().T + bo.double().abs()[None, :] + res.double().abs())
        out = dict(case, np_out=npr, producer=R.worst_ratio(xb, pref, pbound))
        ok_np = 1 <= npr <= 8 and D % npr == 0
        if ok_np:
            width = D // npr
            rec = stats.reshape(-1)[:M * npr * 4].reshape(M, npr, 4).cpu()
            (s, m2, n), (bs, bm) = R.tile_records_ref(xb.double(), width, R.epilogue_record_depth(width))
            out["rec_sum"] = R.worst_ratio(rec[..., 0], s, bs)
            out["rec_m2"] = R.worst_ratio(rec[..., 1], m2, bm)
            out["rec_exact"] = bool((rec[..., 2] == n).all() and (rec[..., 3] == 0).all())
            pad_ok = pad_ok and bool((stats.reshape(-1)[M * npr * 4:] == -7.0).all())
            # ---- the fold of the consumer's weights, on the device (checked on its own in the parent's fold test)
            if (N, D) not in folds:
                W, gamma, beta, b = R.fold_inputs(N, D)
                Wg = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
                sv, cv = torch.empty(N, device=dev), torch.empty(N, device=dev)
                dW, dg, dbeta, db = W.to(dev), gamma.to(dev), beta.to(dev), b.to(dev)
                _lib.check(lib.ec_ln_fold_bf16(dW.data_ptr(), dg.data_ptr(), dbeta.data_ptr(), db.data_ptr(), Wg.data_ptr(),
                                               sv.data_ptr(), cv.data_ptr(), N, D, st), "fold")
                torch.cuda.synchronize()
                folds[(N, D)] = (Wg, sv, cv)
            Wg, sv, cv = folds[(N, D)]
            ref, bound = R.gemm_ln_ref(xb, Wg.cpu(), sv.cpu(), cv.cpu(), act)
            xin = x[:M].contiguous()

            def consume(records, np_):
                y = torch.empty((M + PAD, N), dtype=torch.int16, device=dev)
                y.fill_(SENTINEL)
                _lib.check(lib.ec_gemm_bf16_ln(xin.data_ptr(), Wg.data_ptr(), cv.data_ptr(), None, y.data_ptr(), M, N, D, act,
                                               sv.data_ptr(), records.data_ptr(), np_, None, None, st), "consumer")
                torch.cuda.synchronize()
                yc = y.cpu()
                return R.worst_ratio(yc[:M].view(torch.bfloat16), ref, bound), bool((yc[M:] == SENTINEL).all())

            out["consumer"], p1 = consume(stats, npr)
            one = torch.full((M + PAD, 4), -7.0, dtype=torch.float32, device=dev)
            _lib.check(lib.ec_row_stats_bf16(xin.data_ptr(), one.data_ptr(), M, D, st), "row_stats")
            out["consumer_row_stats"], p2 = consume(one, 1)
            pad_ok = pad_ok and p1 and p2 and bool((one[M:] == -7.0).all())
        out["pad_ok"] = pad_ok
        results.append(out)
    print(json.dumps({"setting": setting, "cases": results}))


if __name__ == "__main__":
    main()
