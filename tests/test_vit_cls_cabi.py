"""The class-embedding entry points on a box without a GPU: the new symbols declared, exported and bound with the header's
argument lists, and every refusal of the three stage entry points and of ec_vit_embed_cls in front of the first HIP call (the
pointers are fake: a check that let a call through would fault here, not return)."""
import ctypes as C
import os
import re

import pytest

NEW = ("ec_vit_cls_workspace_bytes", "ec_vit_embed_cls", "ec_gemm_rows_bf16", "ec_vit_cls_rows_ln", "ec_vit_cls_attn")
OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -4
P = 64        # a non-NULL, 16-byte aligned "pointer": the checks under test return before anything is read
NONE, QUICKGELU = 0, 2


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def test_error_codes_are_the_header_s(repo_root):
    text = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    for name, v in (("EC_OK", OK), ("EC_ERR_ARG", ARG), ("EC_ERR_SHAPE", SHAPE), ("EC_ERR_WORKSPACE", WORKSPACE)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), text), name
    assert re.search(r"\bEC_ACT_QUICKGELU\s*=\s*%d\b" % QUICKGELU, text)


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    from test_cabi_signatures import _agrees, prototypes
    protos = prototypes(repo_root)
    for n in NEW:
        assert n in protos and n in _lib.SIGNATURES and hasattr(lib, n), n
        res, args = _lib.SIGNATURES[n]
        hres, hargs = protos[n]
        assert len(args) == len(hargs) and _agrees(res, hres), n
        assert all(_agrees(a, h) for a, h in zip(args, hargs)), n
    assert protos["ec_vit_cls_workspace_bytes"] == ("size_t", ["ec_vit_t*", "int"])
    assert protos["ec_vit_embed_cls"][1] == ["ec_vit_t*", "float*", "int", "void*", "size_t", "float*", "ec_stream_t"]


def _gemm(lib, A=P, lda=64, W=P, bias=P, res=0, ldr=0, out=P, ldo=32, M=3, N=32, K=64, act=NONE, store=0):
    return lib.ec_gemm_rows_bf16(A, lda, W, bias, res, ldr, out, ldo, M, N, K, act, store, None)


def test_gemm_rows_refusals(lib):
    for kw in (dict(A=0), dict(W=0), dict(out=0)):                                   # NULL
        assert _gemm(lib, **kw) == ARG, kw
    for kw in (dict(A=P + 8), dict(W=P + 2), dict(bias=P + 2), dict(out=P + 1), dict(out=P + 2, store=1), dict(out=P + 2, store=2),
               dict(res=P + 1, ldr=32), dict(store=3), dict(store=-1), dict(act=1), dict(act=7)):   # misaligned, bad enum
        assert _gemm(lib, **kw) == ARG, kw
    for kw in (dict(M=0), dict(M=-1), dict(N=0), dict(N=48), dict(K=0), dict(K=32), dict(K=96), dict(lda=56), dict(lda=68), dict(ldo=31),
               dict(res=P, ldr=31), dict(res=P, ldr=0), dict(lda=-64)):              # shapes and pitches
        assert _gemm(lib, **kw) == SHAPE, kw


def _ln(lib, x=P, pitch=64, gamma=P, beta=P, out=P, rows=3, D=64):
    return lib.ec_vit_cls_rows_ln(x, pitch, gamma, beta, out, rows, D, None)


def test_rows_ln_refusals(lib):
    for kw in (dict(x=0), dict(gamma=0), dict(beta=0), dict(out=0), dict(x=P + 1), dict(out=P + 1), dict(gamma=P + 2), dict(beta=P + 1)):
        assert _ln(lib, **kw) == ARG, kw
    for kw in (dict(rows=0), dict(rows=-2), dict(D=0), dict(D=32), dict(D=96), dict(D=1088), dict(pitch=63), dict(pitch=0), dict(pitch=-64),
               dict(D=128, pitch=64)):
        assert _ln(lib, **kw) == SHAPE, kw


def _attn(lib, q=P, kv=P, out=P, B=2, L=50, D=128, heads=2):
    return lib.ec_vit_cls_attn(q, kv, out, B, L, D, heads, None)


def test_cls_attn_refusals(lib):
    for kw in (dict(q=0), dict(kv=0), dict(out=0), dict(q=P + 1), dict(kv=P + 8), dict(out=P + 1)):
        assert _attn(lib, **kw) == ARG, kw
    for kw in (dict(B=0), dict(B=-1), dict(L=0), dict(L=513), dict(heads=0), dict(heads=4), dict(D=0), dict(D=100), dict(D=192, heads=2)):
        assert _attn(lib, **kw) == SHAPE, kw


def test_embed_cls_refusals(lib):
    """width 64 (one head) has no folded copies, so ec_vit_create issues no HIP call and a handle exists without a GPU"""
    D, layers, patch, res = 64, 2, 32, 64
    L = (res // patch) ** 2 + 1
    n_w = D * patch * patch * 3 + layers * 12 * D * D
    n_f = D + L * D + 2 * D + layers * 13 * D
    h = C.c_void_p()
    assert lib.ec_vit_create(C.byref(h), D, layers, 1, patch, res, P, n_w, P, n_f) == OK
    try:
        assert lib.ec_vit_tokens(h) == L
        assert lib.ec_vit_cls_workspace_bytes(None, 4) == 0 and lib.ec_vit_cls_workspace_bytes(h, 0) == 0
        assert lib.ec_vit_cls_workspace_bytes(h, -3) == 0
        need = lib.ec_vit_cls_workspace_bytes(h, 4)
        # the general route's forward workspace and token stream fit inside it, with the class rows' buffers on top
        assert need >= lib.ec_vit_workspace_bytes(h, 4) + 4 * L * D * 2 + 4 * 9 * D * 2
        assert lib.ec_vit_cls_workspace_bytes(h, 8) > need
        assert lib.ec_vit_embed_cls(None, P, 4, P, need, P, None) == ARG
        assert lib.ec_vit_embed_cls(h, 0, 4, P, need, P, None) == ARG
        assert lib.ec_vit_embed_cls(h, P, 4, 0, need, P, None) == ARG
        assert lib.ec_vit_embed_cls(h, P, 4, P, need, 0, None) == ARG
        assert lib.ec_vit_embed_cls(h, P, 0, P, need, P, None) == SHAPE
        assert lib.ec_vit_embed_cls(h, P, -1, P, need, P, None) == SHAPE
        assert lib.ec_vit_embed_cls(h, P, 4, P, need - 1, P, None) == WORKSPACE
        assert lib.ec_vit_embed_cls(h, P, 4, P, 0, P, None) == WORKSPACE
    finally:
        lib.ec_vit_destroy(h)
