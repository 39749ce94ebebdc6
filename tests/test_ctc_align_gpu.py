"""CTC forced alignment on the MI355X (fk_ctc_align, csrc/ctc.hip) against the float64 restatement tests/ctc_align_ref.py.

Cases: those of tests/ctc_cases.py (a: wave route, L = 0, a single-alignment sample; b31 / b32: the last wave size and the first LDS size,
padded rows; c: S = 511, T = 600, three backtrack chunks; d: C = 50258, two samples without alignment; e: one class in six states) and
the edge family of ctc_align_ref.edge_case (T_b around CTC_ALIGN_PACK and CTC_ALIGN_CHUNK on both routes, the blank in the middle), each
with its random logits and with its planted twin (a unique optimum by a margin of 6 per frame: path, index, start and end are exact).

On the random cases the path must equal the float64 path; a sample may instead pass as a near-tie only if the float64 score of the
device's path is within `tol` of the float64 optimum, at most once over the whole file (tests/test_ctc_align_cpu.py shows that the
recursion in numpy float32 needs that exit zero times).  tol per case: 4 x the error of the float32 numpy restatement against float64
(the kernel's row_lse uses __expf and another summation order), floor 2^-22 max(1, |score|).  A label's sum gets tol scaled to its
share of the frames plus what n frames of row_lse (the bound tests/test_ctc_gpu.py holds it to) and n roundings of the difference and of
the sum may add: n (2^-24 (max |lse| + 4 + C / 64) + 2^-23 max |lp|)."""
import functools

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from tests import ctc_align_ref as A
from tests import ctc_cases as CC
from tests import ctc_ref as R

pytestmark = pytest.mark.gpu

PAD = -100
POISON = 7777
NEAR_TIES = []                                           # (case, sample, float64 optimum, float64 score of the device's path)
KEYS = [(n, d) for n in A.NAMES for d in ("fp32", "bf16")]
IDS = [f"{n}-{d}" for n, d in KEYS]


@functools.lru_cache(maxsize=None)
def refs(name, bf16, planted=False):
    """-> (case, logits fp32 as the kernel sees them, float64 restatement, tol): computed once, shared, read-only"""
    c = A.planted(name) if planted else A.case(name)
    x = c["logits"].to(torch.bfloat16).float() if bf16 else c["logits"]
    args = (x.numpy(), c["targets"].numpy(), c["input_lengths"].numpy(), c["target_lengths"].numpy(), c["blank"])
    r64, r32 = A.viterbi(*args), A.viterbi(*args, dtype=np.float32)
    fin = np.isfinite(r64["score"])
    err32 = float(np.abs(r32["score"].astype(np.float64)[fin] - r64["score"][fin]).max())
    tol = max(4.0 * err32, 2.0 ** -22 * max(1.0, float(np.abs(r64["score"][fin]).max())))
    return c, x, r64, tol, err32


def padded(shape, dtype, fill):
    B, n = shape
    store = torch.full((B, n + 3), fill, dtype=dtype, device="cuda")
    return store, store[:, :n]


def launch(c, x, dtype, il="case", tl="case", targets=None, logits=None, blank=None):
    """fk_ctc_align on the case with padded row strides everywhere -> (numpy outputs, the padding is intact)"""
    B, T, C = x.shape
    if logits is None:
        store = torch.full((B, T, c["ld"]), float("nan"), dtype=dtype, device="cuda")
        store[:, :, :C] = x.to(dtype).cuda()
        logits = store[:, :, :C]
    tg = (c["targets"] if targets is None else targets).cuda()
    il = c["input_lengths"].cuda() if isinstance(il, str) else il
    tl = c["target_lengths"].cuda() if isinstance(tl, str) else tl
    Lmax = tg.shape[1]
    stores, out = {}, {}
    for k, n, dt, fill in (("path", T, torch.int64, POISON), ("index", T, torch.int64, POISON), ("start", Lmax, torch.int64, POISON),
                           ("end", Lmax, torch.int64, POISON), ("label_lp", Lmax, torch.float32, float("nan"))):
        stores[k], out[k] = padded((B, n), dt, fill)
    r = K.ctc_align(logits, tg, il, tl, c["blank"] if blank is None else blank, PAD, PAD, out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in r.items()}
    for k, st in stores.items():
        tail = st[:, out[k].shape[1]:]
        assert bool(torch.isnan(tail).all() if k == "label_lp" else (tail == POISON).all()), f"{k}: the row padding was written"
    return got


@functools.lru_cache(maxsize=None)
def device(name, bf16, planted=False):
    c, x, _, _, _ = refs(name, bf16, planted)
    return launch(c, x, torch.bfloat16 if bf16 else torch.float32)


def consistent(got, ref, blank):
    """what holds for ANY valid alignment: the path collapses to the clamped target, index / start / end describe the path, pad holds
    beyond T_b, a sample without alignment is empty, and nothing is NaN"""
    B, T = got["path"].shape
    assert not np.isnan(got["score"]).any() and not np.isnan(got["label_lp"]).any()
    for b in range(B):
        tb, lb = int(ref["Tb"][b]), int(ref["Lb"][b])
        labels = ref["labels"][b, :lb]
        path, index, start, end = got["path"][b], got["index"][b], got["start"][b], got["end"][b]
        assert (start[lb:] == -1).all() and (end[lb:] == -1).all() and not got["label_lp"][b, lb:].any()
        assert (path[tb:] == PAD).all() and (index[tb:] == -1).all()
        if np.isneginf(ref["score"][b]):
            assert np.isneginf(got["score"][b]) and (path == PAD).all() and (index == -1).all()
            assert (start == -1).all() and (end == -1).all() and not got["label_lp"][b].any()
            continue
        assert np.isfinite(got["score"][b])
        ids, lens = R.collapse(path[None, :tb], None, blank) if tb else (np.zeros((1, 0)), [0])
        assert lens[0] == lb and ids[0, :lb].tolist() == labels.tolist(), (b, "the path does not collapse to the target")
        assert ((index[:tb] == -1) == (path[:tb] == blank)).all()
        at = 0
        for i in range(lb):
            s, e = int(start[i]), int(end[i])
            assert at <= s < e <= tb and (index[s:e] == i).all() and (path[s:e] == labels[i]).all(), (b, i, s, e)
            assert (index[at:s] == -1).all()
            at = e
        assert (index[at:tb] == -1).all()


def same_path_or_near_tie(name, got, ref, tol):
    for b in range(len(ref["score"])):
        if np.array_equal(got["path"][b], ref["path"][b]):
            for k in ("index", "start", "end"):
                assert np.array_equal(got[k][b], ref[k][b]), (name, b, k)
            continue
        tb = int(ref["Tb"][b])
        mine = A.path_score(ref["lp"][b], got["path"][b], tb)
        print(f"ctc align {name} sample {b}: the device's path differs; float64 optimum {ref['score'][b]:.9f}, the device's path {mine:.9f}, tol {tol:.3e}")
        assert ref["score"][b] - mine <= tol, (name, b, "a worse path, not a near-tie")
        NEAR_TIES.append((name, b, float(ref["score"][b]), float(mine)))
        assert len(NEAR_TIES) <= 1, NEAR_TIES


@pytest.mark.parametrize("name,dt", KEYS, ids=IDS)
def test_planted_alignment_is_exact(name, dt):
    c, x, ref, tol, _ = refs(name, dt == "bf16", True)
    got = device(name, dt == "bf16", True)
    consistent(got, ref, c["blank"])
    for k in ("path", "index", "start", "end"):
        assert np.array_equal(got[k], ref[k]), (name, dt, k)
    for b, st in enumerate(c["planted"]):
        if st is not None:
            assert np.array_equal(got["path"][b, :len(st)], R.extended(ref["labels"][b, :ref["Lb"][b]], c["blank"])[st])


@pytest.mark.parametrize("name,dt", KEYS, ids=IDS)
def test_random_path_is_the_float64_path(name, dt):
    c, x, ref, tol, _ = refs(name, dt == "bf16")
    got = device(name, dt == "bf16")
    assert K.ctc_route(c["targets"].shape[1]) == (K._lib.CTC_WAVE if 2 * c["targets"].shape[1] + 1 <= 64 else K._lib.CTC_LDS)
    consistent(got, ref, c["blank"])
    assert int(np.isneginf(got["score"]).sum()) == c["infeasible"]
    same_path_or_near_tie(f"{name}-{dt}", got, ref, tol)


@pytest.mark.parametrize("planted", [False, True], ids=["random", "planted"])
@pytest.mark.parametrize("name,dt", KEYS, ids=IDS)
def test_scores(name, dt, planted):
    bf16 = dt == "bf16"
    c, x, ref, tol, err32 = refs(name, bf16, planted)
    got = device(name, bf16, planted)
    fin = np.isfinite(ref["score"])
    assert np.array_equal(np.isneginf(got["score"]), ~fin)
    err = float(np.abs(got["score"].astype(np.float64)[fin] - ref["score"][fin]).max())
    B, T, C = x.shape
    lp_fin = ref["lp"][np.isfinite(ref["lp"])]
    per_frame = 2.0 ** -24 * (float(np.abs(ref["lse"]).max()) + 4 + C / 64) + 2.0 ** -23 * float(np.abs(lp_fin).max())
    worst, worst_tol, margin = 0.0, 0.0, -np.inf               # the label closest to (or furthest past) its tolerance
    for b in np.nonzero(fin)[0]:
        for i in range(int(ref["Lb"][b])):
            s, e = int(got["start"][b, i]), int(got["end"][b, i])
            want = A.path_score(ref["lp"][b, s:e], np.full(e - s, ref["labels"][b, i]), e - s)          # float64, the same span
            d = abs(float(got["label_lp"][b, i]) - want)
            t = tol * (e - s) / int(ref["Tb"][b]) + (e - s) * per_frame
            if d - t > margin:
                worst, worst_tol, margin = d, t, d - t
            assert d <= t, (name, dt, b, i, d, t)
    # score <= -nll of the loss on the same inputs, up to this tolerance and the loss's own (tests/test_ctc_gpu.py: 4 x torch's fp32 error)
    nll64 = R.ctc(x.numpy(), c["targets"].numpy(), c["input_lengths"].numpy(), c["target_lengths"].numpy(), blank=c["blank"])["raw"]
    nll32, _ = CC.torch_ctc(c, torch.float32, "none", False, logits=x)
    tol_nll = max(4.0 * float(np.abs(nll32.numpy().astype(np.float64)[fin] - nll64[fin]).max()), 8.0 * 2.0 ** -24 * max(1.0, float(np.abs(nll64[fin]).max())))
    store = torch.full((B, T, c["ld"]), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    store[:, :, :C] = x.cuda()
    nll = K.ctc_loss_fwd(store[:, :, :C], c["targets"].cuda(), c["input_lengths"].cuda(), c["target_lengths"].cuda(), c["blank"], "none", False,
                         want_grad=False).nll.cpu().numpy().astype(np.float64)
    print(f"ctc align scores {name}-{dt} {'planted' if planted else 'random'}: |float32 numpy - f64| {err32:.3e}  |kernel - f64| {err:.3e} (tol {tol:.3e});  "
          f"label_lp worst |kernel - f64| {worst:.3e} (tol {worst_tol:.3e});  max |score| {np.abs(ref['score'][fin]).max():.1f};  tol nll {tol_nll:.3e}")
    assert err <= tol, (name, dt, err, tol)
    assert np.array_equal(np.isposinf(nll), ~fin)
    assert np.all(got["score"][fin] <= -nll[fin] + tol + tol_nll), (got["score"], -nll)


# ---- exact statements ---------------------------------------------------------------------------------------------------------------
def differing(a, b):
    """the outputs whose bits differ (none: [])"""
    return [k for k in ("score", "path", "index", "start", "end", "label_lp") if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("name", ["a", "b32", "d", "edge65"])
def test_lengths_none_optional_outputs_strides_and_two_runs(name):
    c, x, ref, tol, _ = refs(name, False)
    got = device(name, False)
    # two runs: the same bits
    assert not differing(launch(c, x, torch.float32), got)
    # target_lengths None: the padding is counted on the device
    assert not differing(launch(c, x, torch.float32, tl=None), got)
    # input_lengths None: T frames each
    B, T, C = x.shape
    full = launch(c, x, torch.float32, il=torch.full((B,), T, dtype=torch.int64, device="cuda"))
    assert not differing(launch(c, x, torch.float32, il=None), full)
    # a batch stride beyond T rows (four rows more: every row keeps its offset from a 16-byte boundary, on which the order of the sums
    # in row_lse, and so the last bits of the scores, depend)
    store = torch.full((B, T + 4, c["ld"]), float("nan"), device="cuda")
    store[:, :T, :C] = x.cuda()
    lg = store[:, :T, :C]
    assert lg.stride(0) == (T + 4) * c["ld"] and not lg.is_contiguous()
    assert not differing(launch(c, x, torch.float32, logits=lg), got)
    # optional outputs left out: score and path keep their bits (the guard bands of the autouse fixture hold stray writes)
    tg, il, tl = c["targets"].cuda(), c["input_lengths"].cuda(), c["target_lengths"].cuda()
    r = K.ctc_align(lg, tg, il, tl, c["blank"], PAD, PAD, want_index=False, want_spans=False)
    assert r["index"] is None and r["start"] is None and r["end"] is None and r["label_lp"] is None
    assert np.array_equal(r["score"].cpu().numpy(), got["score"]) and np.array_equal(r["path"].cpu().numpy(), got["path"])
    r = K.ctc_align(lg, tg, il, tl, c["blank"], PAD, PAD, want_index=False)
    assert r["index"] is None and np.array_equal(r["start"].cpu().numpy(), got["start"]) and np.array_equal(r["label_lp"].cpu().numpy(), got["label_lp"])


@pytest.mark.parametrize("name", ["a", "b32"])
def test_clamped_labels_and_lengths_match_the_reference_under_the_same_clamp(name):
    """a label past the classes, a label equal to the blank, a negative label, lengths past the buffers and below zero"""
    c, x, _, _, _ = refs(name, False)
    B, T, C = x.shape
    tg, il, tl = c["targets"].clone(), c["input_lengths"].clone(), c["target_lengths"].clone()
    tg[0, 0], tg[0, 1], tg[B - 1, 0] = C + 7, c["blank"], -5
    il[0], tl[0], il[B - 1] = T + 5, tg.shape[1] + 3, -2
    for tlen in (tl, None):
        args = (x.numpy(), tg.numpy(), il.numpy(), None if tlen is None else tlen.numpy(), c["blank"])
        ref, r32 = A.viterbi(*args), A.viterbi(*args, dtype=np.float32)
        fin = np.isfinite(ref["score"])
        tol = max(4.0 * float(np.abs(r32["score"].astype(np.float64)[fin] - ref["score"][fin]).max()), 2.0 ** -22 * max(1.0, float(np.abs(ref["score"][fin]).max())))
        got = launch(c, x, torch.float32, il=il.cuda(), tl=None if tlen is None else tlen.cuda(), targets=tg)
        consistent(got, ref, c["blank"])
        same_path_or_near_tie(f"{name}-clamped", got, ref, tol)
        assert float(np.abs(got["score"].astype(np.float64)[fin] - ref["score"][fin]).max()) <= tol


def test_graph_capture_replays_the_same_bits():
    """the two launches inside a stream capture (which raises on anything that waits for the host), padded targets counted on the device"""
    c, x, _, _, _ = refs("b32", False)
    got = device("b32", False)
    lg, tg, il = x.cuda(), c["targets"].cuda(), c["input_lengths"].cuda()

    def step():
        return E.ctc_forced_align(lg, tg, il, None, blank=c["blank"])

    r0 = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r1 = step()
    graph.replay()
    torch.cuda.synchronize()
    for k in ("score", "path", "index", "start", "end", "label_lp"):
        assert torch.equal(getattr(r1, k), getattr(r0, k)), k
        assert np.array_equal(getattr(r1, k).cpu().numpy(), got[k]), k
    conf = r1.confidence.cpu().numpy()
    n = np.maximum(got["end"] - got["start"], 1)
    want = np.where(got["end"] > got["start"], np.exp(got["label_lp"] / n), 0.0)
    np.testing.assert_allclose(conf, want, rtol=1e-5, atol=0)
    assert ((conf >= 0) & (conf <= 1)).all()


# ---- model ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def test_model_align(fp32_mode):
    """BrainFormerCTC.align on the small model of test_ctc_gpu.test_model_loss_gradients_and_decoding; aligning the greedy decode of a
    planted input returns spans whose collapse is that decode"""
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    enc = bf.MAEConfig(window_size=200, n_electrodes=64, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512, n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=8, output_dim=6, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)
    torch.manual_seed(3)
    m = BrainFormerCTC(cfg).cuda()
    with torch.no_grad():
        m.perceiver["to_words"].weight.normal_(0.0, 0.5)
    x = torch.randn(2, 200, 64, device="cuda")
    targets = torch.tensor([[1, 1, 2, -100], [3, 0, 4, 2]], device="cuda")
    with torch.no_grad():
        logits = m.features(x)
    got = m.align(x, targets)
    want = E.ctc_forced_align(logits, targets, blank=m.blank)
    for k in ("score", "path", "index", "start", "end", "label_lp"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    ref = A.viterbi(logits.float().cpu().numpy(), targets.cpu().numpy(), None, None, m.blank)
    consistent({k: getattr(got, k).cpu().numpy() for k in ("score", "path", "index", "start", "end", "label_lp")}, ref, m.blank)
    assert np.abs(got.score.cpu().numpy() - ref["score"]).max() < 1e-4
    # a planted input: the greedy decode is the planted labelling, and its alignment collapses to it
    c = A.planted("a")
    lg = c["logits"].contiguous().cuda()
    il = c["input_lengths"].cuda()
    ids, lens = E.ctc_greedy_decode(lg, il, blank=c["blank"])
    Lmax = int(lens.max())
    al = E.ctc_forced_align(lg, ids[:, :Lmax], il, lens, blank=c["blank"])
    assert bool(torch.isfinite(al.score).all())
    back, back_lens = E.ctc_greedy_decode(torch.nn.functional.one_hot(al.path.clamp(min=0), lg.shape[2]).float() * 9.0, il, blank=c["blank"])
    assert torch.equal(back_lens, lens) and torch.equal(back[:, :Lmax], ids[:, :Lmax])
    for b in range(lg.shape[0]):
        for i in range(int(lens[b])):
            s, e = int(al.start[b, i]), int(al.end[b, i])
            assert e > s and bool((al.path[b, s:e] == ids[b, i]).all())
    # greedy's path is the best path: the planted frames
    argmax = lg.argmax(-1)
    for b in range(lg.shape[0]):
        tb = int(il[b])
        assert torch.equal(al.path[b, :tb], argmax[b, :tb])


def test_near_tie_exits_at_most_one():
    print(f"ctc align: near-tie exits over the file: {NEAR_TIES}")
    assert len(NEAR_TIES) <= 1
