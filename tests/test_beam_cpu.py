"""CPU-side checks of the beam-search entry points (csrc/decode.hip): fk_attn_decode_beam, fk_beam_topk and fk_beam_select are exported and
bound, and each refuses what lies outside its declared envelope on the host, with FK_EINVAL and before any launch (the pointers below are
small fake addresses: a call that got past the checks would fault, so every call here has exactly one thing wrong with it and nothing that
would be valid)."""
import ctypes

import pytest

EINVAL = -1
P = 4096          # a fake, 16-byte aligned "device pointer": never dereferenced by a refused call


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_exports_exist(lib):
    from frankenstein_amd import _lib
    h = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("fk_attn_decode_beam", "fk_beam_topk", "fk_beam_select"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    from frankenstein_amd import kernels as K
    assert callable(K.attn_decode_beam) and callable(K.beam_topk) and callable(K.beam_select) and K.BeamState
    assert (K.BEAM_MAX_WIDTH, K.BEAM_MAX_TOPK) == (16, 64)


def attn(lib, q=P, kv=P, anc=P, out=P, pos=P, W=5, H=2, D=64, kv_bs=320 * 256, kv_rs=256, dtype=1):
    return lib.fk_attn_decode_beam(q, 3 * H * D, kv, kv_bs, kv_rs, anc, 320, out, H * D, pos, W, H, D, 0.125, dtype, None)


def test_attn_decode_beam_refuses_bad_arguments(lib):
    for name in ("q", "kv", "anc", "out", "pos"):
        assert attn(lib, **{name: None}) == EINVAL, name
        assert b"fk_attn_decode_beam" in lib.fk_last_error()
    assert attn(lib, D=48, kv_rs=2 * 2 * 48, kv_bs=320 * 192) == EINVAL and b"head_dim 48" in lib.fk_last_error()
    assert attn(lib, D=0) == EINVAL
    assert attn(lib, W=0) == EINVAL
    assert attn(lib, H=0) == EINVAL
    assert attn(lib, dtype=7) == EINVAL
    assert attn(lib, kv=P + 4) == EINVAL and b"16-byte" in lib.fk_last_error()       # rows are read as 16-byte vectors
    assert attn(lib, kv_rs=260) == EINVAL and b"16-byte" in lib.fk_last_error()
    assert attn(lib, kv_rs=128) == EINVAL                                            # a row shorter than key | value


def topk(lib, logits=P, ld=211, R=5, V=211, temperature=1.0, k=20, top_lp=P, top_id=P):
    return lib.fk_beam_topk(logits, ld, R, V, temperature, k, top_lp, top_id, None)


def test_beam_topk_refuses_bad_arguments(lib):
    for name in ("logits", "top_lp", "top_id"):
        assert topk(lib, **{name: None}) == EINVAL and b"fk_beam_topk: null pointer" in lib.fk_last_error(), name
    for k in (0, -1, 65):
        assert topk(lib, k=k) == EINVAL and b"fk_beam_topk: k=" in lib.fk_last_error(), k
    assert topk(lib, V=10, ld=10, k=11) == EINVAL and b"fk_beam_topk: k=11" in lib.fk_last_error()          # k > V
    assert topk(lib, ld=210) == EINVAL and b"ld=210" in lib.fk_last_error()                                    # ld < V
    for t in (0.0, -1.0):
        assert topk(lib, temperature=t) == EINVAL and b"temperature" in lib.fk_last_error(), t
    assert topk(lib, R=0) == EINVAL
    assert topk(lib, V=0, ld=0) == EINVAL
    assert topk(lib, V=1 << 31, ld=1 << 31) == EINVAL                                                          # V < 2^31


def select(lib, top_lp=P, top_id=P, row_stride=None, W=5, k=20, scores=P, seed=P, step=P, pos=P, pos_inc=P, cur=P, parent_log=P, tok_log=P,
           log_rows=8, anc=P, anc_ld=320):
    return lib.fk_beam_select(top_lp, top_id, k if row_stride is None else row_stride, W, k, scores, seed, step, pos, pos_inc, cur, parent_log,
                              tok_log, log_rows, anc, anc_ld, None)


def test_beam_select_refuses_bad_arguments(lib):
    for name in ("top_lp", "top_id", "scores", "seed", "step", "pos", "cur", "anc"):
        assert select(lib, **{name: None}) == EINVAL and b"fk_beam_select: null pointer" in lib.fk_last_error(), name
    for W, k in ((0, 20), (17, 20), (17, 64), (5, 4), (16, 15), (5, 65), (5, 0)):          # W = 0, W = 17, W > k, k = 65, k = 0
        assert select(lib, W=W, k=k) == EINVAL and b"fk_beam_select: need 1 <= W <= 16 and W <= k <= 64" in lib.fk_last_error(), (W, k)
    assert select(lib, row_stride=19) == EINVAL                                           # rows that overlap
    assert select(lib, anc_ld=0) == EINVAL
    assert select(lib, parent_log=None) == EINVAL and select(lib, tok_log=None) == EINVAL  # logs announced (log_rows = 8) but absent
    assert select(lib, log_rows=-1) == EINVAL
