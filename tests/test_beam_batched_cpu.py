"""CPU-side checks of the batched beam-search entry points (csrc/decode.hip): fk_attn_decode_beam_grouped and fk_beam_select_grouped are
exported and bound, and each refuses what lies outside its declared envelope on the host, with FK_EINVAL and before any launch (the
pointers below are small fake addresses: a call that got past the checks would fault, so every call here has exactly one thing wrong with
it and nothing that would be valid)."""
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
    for name in ("fk_attn_decode_beam_grouped", "fk_beam_select_grouped"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["fk_attn_decode_beam_grouped"][1]) == 19 and len(_lib.SIGNATURES["fk_beam_select_grouped"][1]) == 20
    from frankenstein_amd import kernels as K
    assert callable(K.attn_decode_beam_grouped) and callable(K.beam_select_grouped)


def attn(lib, q=P, kv=P, anc=P, out=P, pos=P, S=3, W=5, H=2, D=64, q_bs=None, kv_bs=320 * 256, kv_rs=256, tmax=320, append=1, dtype=1):
    return lib.fk_attn_decode_beam_grouped(q, 3 * H * D if q_bs is None else q_bs, kv, kv_bs, kv_rs, tmax, anc, 320, out, H * D, pos, S, W, H, D,
                                           0.125, append, dtype, None)


def test_attn_decode_beam_grouped_refuses_bad_arguments(lib):
    for name in ("q", "kv", "anc", "out", "pos"):
        for append in (0, 1):
            assert attn(lib, append=append, **{name: None}) == EINVAL, name
            assert b"fk_attn_decode_beam_grouped" in lib.fk_last_error()
    assert attn(lib, S=0) == EINVAL and b"S >= 1" in lib.fk_last_error()
    assert attn(lib, S=-1) == EINVAL
    assert attn(lib, S=4096, W=16) == EINVAL and b"S * W < 65536" in lib.fk_last_error()       # 65536 rows: past the grid's y extent
    assert attn(lib, S=65536, W=1) == EINVAL
    assert attn(lib, W=0) == EINVAL
    assert attn(lib, H=0) == EINVAL
    assert attn(lib, D=48, kv_rs=2 * 2 * 48, kv_bs=320 * 192) == EINVAL and b"head_dim 48" in lib.fk_last_error()
    assert attn(lib, D=0) == EINVAL
    assert attn(lib, dtype=7) == EINVAL
    assert attn(lib, tmax=0) == EINVAL and b"tmax=0" in lib.fk_last_error()
    assert attn(lib, tmax=-3) == EINVAL
    for append in (0, 1):
        assert attn(lib, kv=P + 4, append=append) == EINVAL and b"16-byte" in lib.fk_last_error()    # rows are read as 16-byte vectors
        assert attn(lib, kv_rs=260, append=append) == EINVAL and b"16-byte" in lib.fk_last_error()
        assert attn(lib, kv_rs=128, append=append) == EINVAL                                          # a row shorter than key | value
    # the append path reads the new key | value row of qkv as 16-byte vectors
    assert attn(lib, q=P + 4) == EINVAL and b"append" in lib.fk_last_error()
    assert attn(lib, q_bs=3 * 128 + 4) == EINVAL and b"append" in lib.fk_last_error()
    assert attn(lib, q_bs=128) == EINVAL and b"append" in lib.fk_last_error()                       # a row that holds only q


def select(lib, top_lp=P, top_id=P, row_stride=None, group_stride=None, S=3, W=5, k=20, scores=P, seed=P, step=P, pos=P, pos_inc=P, cur=P,
           parent_log=P, tok_log=P, log_rows=8, anc=P, anc_ld=320, ticket=P):
    rs = k if row_stride is None else row_stride
    gs = W * max(rs, k) if group_stride is None else group_stride
    return lib.fk_beam_select_grouped(top_lp, top_id, rs, gs, S, W, k, scores, seed, step, pos, pos_inc, cur, parent_log, tok_log, log_rows, anc,
                                      anc_ld, ticket, None)


def test_beam_select_grouped_refuses_bad_arguments(lib):
    for name in ("top_lp", "top_id", "scores", "seed", "step", "pos", "cur", "anc", "ticket"):
        assert select(lib, **{name: None}) == EINVAL and b"fk_beam_select_grouped: null pointer" in lib.fk_last_error(), name
    for W, k in ((0, 20), (17, 20), (17, 64), (5, 4), (16, 15), (5, 65), (5, 0)):          # W = 0, W = 17, W > k, k = 65, k = 0
        assert select(lib, W=W, k=k) == EINVAL and b"fk_beam_select_grouped: need 1 <= W <= 16 and W <= k <= 64" in lib.fk_last_error(), (W, k)
    assert select(lib, S=0) == EINVAL and b"S >= 1" in lib.fk_last_error()
    assert select(lib, S=-2) == EINVAL
    assert select(lib, S=4096, W=16) == EINVAL and b"S * W < 65536" in lib.fk_last_error()
    assert select(lib, row_stride=19) == EINVAL and b"overlap" in lib.fk_last_error()        # a beam's row runs into the next beam's
    assert select(lib, group_stride=5 * 20 - 1) == EINVAL and b"overlap" in lib.fk_last_error()  # a sentence's rows run into the next sentence's
    assert select(lib, row_stride=0, group_stride=19) == EINVAL and b"overlap" in lib.fk_last_error()   # first step: one row of k per sentence
    assert select(lib, row_stride=24, group_stride=4 * 24 + 19) == EINVAL                    # the last row needs k entries, not row_stride
    assert select(lib, anc_ld=0) == EINVAL
    assert select(lib, parent_log=None) == EINVAL and select(lib, tok_log=None) == EINVAL    # logs announced (log_rows = 8) but absent
    assert select(lib, log_rows=-1) == EINVAL
