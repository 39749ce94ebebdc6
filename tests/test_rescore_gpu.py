"""LM rescoring of n-best lists on the MI355X (csrc/rescore.hip, GPT.score_nbest / rescore_nbest) against the float64 restatement
tests/rescore_ref.py, on the cases of tests/rescore_cases.py.

The index arrays (trie, head rows, visibility table, order, ids, lengths, n_scored) must equal the restatement's exactly: every ranking
case carries a margin of 16 * e32 between the totals the ranking separates.  A log-probability gets max(4 * e32, 8 * 2^-24 * max(1, |lm|)),
the rule of tests/test_ctc_beam_gpu.py (e32: what float32 arithmetic costs the flat restatement itself on that case); a total gets
|lm_weight| times that plus 8 * 2^-24 * max(1, |total|) for its own two multiplies and adds.  In bf16 mode the yardstick is the flat scoring
through GPT.forward measured in the same test: the packed error may be 4 x that (independent roundings of the same size).  The errors are
printed (profiles/lm_rescore.md records them)."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import _lib
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
from tests import rescore_cases as RC
from tests import rescore_ref as RR

pytestmark = pytest.mark.gpu

ALL = list(RC.CASES)
_MODELS = {}


@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def model(V):
    """the test model of tests/rescore_cases.py on the GPU (fp32 masters holding the state dict's values), one per vocabulary"""
    if V not in _MODELS:
        cfg = RC.gpt_cfg(V)
        m = GPT(GPTConfig(block_size=cfg.block_size, vocab_size=V, n_layer=cfg.n_layer, n_head=cfg.n_head, n_embd=cfg.n_embd, bias=True)).cuda().eval()
        own = m.state_dict()
        with torch.no_grad():
            for k, v in RC.state_dict(V).items():
                own[k].copy_(v)
        E.bump_weight_epoch()
        _MODELS[V] = m
    return _MODELS[V]


def on_gpu(case):
    """the case's inputs on the device; ids keep their strides and the garbage around them"""
    inp = case["inp"]
    B, n, T = inp.ids.shape
    store = torch.full((B, n + 1, T + 3), RC.GARBAGE, dtype=torch.int64, device="cuda")
    store[:, :n, :T] = inp.ids.cuda()
    return store[:, :n, :T], inp.lengths.cuda(), inp.am.cuda(), None if inp.prefix is None else inp.prefix.cuda()


def stack(case, key):
    return np.stack([tr[key] for tr in case["tries"]])


def flat_on_gpu(m, case):
    """the flat scoring a user writes from GPT.forward: per sentence the n hypotheses as rows [bos, tokens, padding] behind the repeated
    prefix, all logits, log_softmax, gather, sum -> lm [B, n] (float64 on the host; NaN where the restatement has -inf)"""
    ids, lengths, _, prefix = on_gpu(case)
    B, n, T = ids.shape
    V = case["V"]
    lens = lengths.clamp(0, T)
    out = np.full((B, n), np.nan)
    for b in range(B):
        tok = ids[b].clone()
        tok[(tok < 0) | (tok >= V)] = 0                                                # padding and bad tokens: rows / positions nobody reads
        idx = torch.cat([torch.full((n, 1), case["bos"], dtype=torch.int64, device="cuda"), tok], dim=1)
        pf = None if prefix is None else prefix[b:b + 1].expand(n, -1, -1).contiguous()
        with torch.no_grad():
            _, logits = m(idx, prefix=pf, targets=idx)
        logp = torch.log_softmax(logits.float(), dim=-1)                               # [n, 1 + T, V]
        nxt = logp[:, :-1].gather(2, tok[:, :, None])[:, :, 0]                         # log p(token j | ...), j < T
        keep = torch.arange(T, device="cuda")[None, :] < lens[b][:, None]
        lm = (nxt * keep).double().sum(1)
        if case["eos"] is not None:
            lm = lm + logp[torch.arange(n, device="cuda"), lens[b], case["eos"]].double()
        out[b] = lm.cpu().numpy()
    out[~np.isfinite(case["lm"])] = np.nan
    return out


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_trie_and_mask_are_exact(name):
    case = RC.make(name)
    ids, lengths, am, _ = on_gpu(case)
    n, T, P, N, V = case["n"], case["T"], case["P"], case["N"], case["V"]
    sizing = K.nbest_trie(ids, lengths, am, V, case["bos"], case["eos"], 1 + n * T, P, heads=False)
    if case["max_nodes"] is None:
        want = [RR.trie(case["inp"].ids.numpy()[b], case["inp"].lengths.numpy()[b], case["inp"].am.numpy()[b], V, case["bos"], 1 + n * T)["n_nodes"]
                for b in range(case["B"])]
        assert sizing.n_nodes.cpu().tolist() == want and sizing.head_src is None
        assert RC.node_rows(P, max(want)) == N
    t = K.nbest_trie(ids, lengths, am, V, case["bos"], case["eos"], N, P)
    for key in ("tok", "depth", "parent", "leaf"):
        assert np.array_equal(getattr(t, key).cpu().numpy(), stack(case, key)), (name, key)
    assert t.n_nodes.cpu().tolist() == [tr["n_nodes"] for tr in case["tries"]]
    heads = [RR.head_rows(tr, n, P, case["eos"]) for tr in case["tries"]]
    assert np.array_equal(t.head_src.cpu().numpy(), np.stack([h[0] for h in heads])), name
    assert np.array_equal(t.head_tgt.cpu().numpy(), np.stack([h[1] for h in heads])), name
    mask = K.nbest_trie_mask(t.parent, t.n_nodes, P)
    assert mask.kind == K.MASK_DENSE and mask.limits.shape == (case["B"], 1, P + N, P + N)
    assert np.array_equal(mask.limits[:, 0].cpu().numpy(), np.stack([RR.visibility(tr, P) for tr in case["tries"]])), name
    # no acoustic scores: every slot is present
    t0 = K.nbest_trie(ids, lengths, None, V, case["bos"], case["eos"], N, P)
    ref0 = [RR.trie(case["inp"].ids.numpy()[b], case["inp"].lengths.numpy()[b], None, V, case["bos"], N) for b in range(case["B"])]
    assert np.array_equal(t0.leaf.cpu().numpy(), np.stack([r["leaf"] for r in ref0]))


def _random_list(n, T, V, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, V - 1, size=(1, n, T))
    ids[0, 1::2, :T // 2] = ids[0, 0::2, :T // 2]                                       # pairs share their first half
    return ids, np.full((1, n), T, dtype=np.int64)


def test_the_edges_of_the_envelope():
    """T = FK_NBEST_MAX_T with node_cap = FK_NBEST_MAX_NODES (the worst case of the largest list fits exactly), and the visibility table
    at P + N = FK_NBEST_MAX_ROWS with a list that overflows N"""
    V = 307
    ids, lengths = _random_list(32, _lib.NBEST_MAX_T, V, 1)
    want = RR.trie(ids[0], lengths[0], None, V, V - 1, _lib.NBEST_MAX_NODES)
    t = K.nbest_trie(torch.from_numpy(ids).cuda(), torch.from_numpy(lengths).cuda(), None, V, V - 1, None, _lib.NBEST_MAX_NODES, 0)
    for key in ("tok", "depth", "parent", "leaf"):
        assert np.array_equal(getattr(t, key).cpu().numpy()[0], want[key]), key
    assert int(t.n_nodes[0]) == want["n_nodes"] > 16 * _lib.NBEST_MAX_T and np.all(want["leaf"] > 0)
    P = 16
    N = _lib.NBEST_MAX_ROWS - P
    ids, lengths = _random_list(32, 200, V, 2)
    want = RR.trie(ids[0], lengths[0], None, V, V - 1, N)
    assert (want["leaf"] < 0).any() and (want["leaf"] > 0).any()
    t = K.nbest_trie(torch.from_numpy(ids).cuda(), torch.from_numpy(lengths).cuda(), None, V, V - 1, 5, N, P)
    assert np.array_equal(t.parent.cpu().numpy()[0], want["parent"]) and np.array_equal(t.leaf.cpu().numpy()[0], want["leaf"])
    mask = K.nbest_trie_mask(t.parent, t.n_nodes, P)
    assert np.array_equal(mask.limits[0, 0].cpu().numpy(), RR.visibility(want, P))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_pos(dtype):
    case = RC.make("edits")
    m = model(case["V"])
    P, N = case["P"], case["N"]
    tok = torch.from_numpy(stack(case, "tok")).to(torch.int32).cuda()
    depth = torch.from_numpy(stack(case, "depth")).to(torch.int32).cuda()
    prefix = case["inp"].prefix.cuda().to(dtype)
    wte, wpe = m.transformer.wte.weight.detach(), m.transformer.wpe.weight.detach()
    got = K.gpt_embed_pos(tok, depth, prefix, wte, wpe, dtype)
    want = torch.cat([prefix.float() + wpe[:P], wte[tok.long()] + wpe[P + depth.long()]], dim=1).to(dtype)
    assert got.shape == (case["B"], P + N, 128) and torch.equal(got, want)
    got0 = K.gpt_embed_pos(tok, depth, None, wte, wpe, dtype)
    assert torch.equal(got0, (wte[tok.long()] + wpe[depth.long()]).to(dtype))


# ---- scores -----------------------------------------------------------------------------------------------------------------------------
def _kwargs(case):
    return dict(bos_token_id=case["bos"], eos_token_id=case["eos"], max_nodes=case["max_nodes"])


@pytest.mark.parametrize("name", ALL)
def test_score_nbest_fp32(name, fp32_mode):
    case = RC.make(name)
    m = model(case["V"])
    ids, lengths, am, prefix = on_gpu(case)
    lm, n_nodes = m.score_nbest(ids, lengths, prefix=prefix, am_scores=am, **_kwargs(case))
    assert lm.dtype == torch.float32 and lm.shape == (case["B"], case["n"]) and n_nodes.cpu().tolist() == [tr["n_nodes"] for tr in case["tries"]]
    lm = lm.cpu().numpy().astype(np.float64)
    fin = np.isfinite(case["lm"])
    assert np.all(np.isneginf(lm[~fin]))
    tol = RC.tolerance(case["e32"], case["lm"])[fin]
    err = np.abs(lm[fin] - case["lm"][fin])
    flat = flat_on_gpu(m, case)
    err_flat = np.abs(lm[fin] - flat[fin])
    print(f"rescore {name:9s} fp32: e32 {case['e32']:.3e}  |packed - f64| {err.max():.3e}  |packed - flat on the GPU| {err_flat.max():.3e}  "
          f"|flat on the GPU - f64| {np.abs(flat[fin] - case['lm'][fin]).max():.3e}  largest error / tolerance {(err / tol).max():.2f}")
    assert np.all(err <= tol), (name, err.max(), (err / tol).max())
    assert np.all(err_flat <= tol), (name, err_flat.max(), (err_flat / tol).max())


@pytest.mark.parametrize("name", ["edits", "wide", "big"])
def test_score_nbest_bf16(name):
    """bf16 mode: the flat scoring through today's GPT.forward against float64 is the yardstick; packed may be 4 x as far off"""
    case = RC.make(name)
    m = model(case["V"])
    ids, lengths, am, prefix = on_gpu(case)
    assert E.compute_dtype() == torch.bfloat16
    lm, _ = m.score_nbest(ids, lengths, prefix=prefix, am_scores=am, **_kwargs(case))
    lm = lm.cpu().numpy().astype(np.float64)
    fin = np.isfinite(case["lm"])
    assert np.all(np.isneginf(lm[~fin]))
    flat_err = np.abs(flat_on_gpu(m, case)[fin] - case["lm"][fin]).max()
    packed_err = np.abs(lm[fin] - case["lm"][fin]).max()
    print(f"rescore {name:9s} bf16: |flat through GPT.forward - f64| {flat_err:.3e}  |packed - f64| {packed_err:.3e}  max |lm| {np.abs(case['lm'][fin]).max():.1f}")
    assert packed_err <= 4.0 * flat_err, (name, packed_err, flat_err)


def check_ranked(case, got, label):
    """order, ids, lengths and n_scored exact; lm and total within tolerance; unscored slots -inf and last"""
    ids, lengths, am, lm, total, order, n_scored = (t.cpu().numpy() for t in got)
    B, n, T = case["B"], case["n"], case["T"]
    assert ids.dtype == lengths.dtype == order.dtype == n_scored.dtype == np.int64 and lm.dtype == total.dtype == am.dtype == np.float32
    assert np.array_equal(order, case["order"]), (label, order, case["order"])
    assert np.array_equal(n_scored, case["n_scored"]), label
    src_ids, src_len, src_am = case["inp"].ids.numpy(), RR.clamp_lengths(case["inp"].lengths.numpy(), T), case["inp"].am.numpy()
    lw = case["weights"][1]
    for b in range(B):
        o = case["order"][b]
        assert np.array_equal(lengths[b], src_len[b][o]) and np.array_equal(am[b], src_am[b][o]), (label, b)
        for r in range(n):
            L = src_len[b][o[r]]
            assert np.array_equal(ids[b, r, :L], src_ids[b, o[r], :L]) and np.all(ids[b, r, L:] == -100), (label, b, r)
        ns = case["n_scored"][b]
        assert np.all(np.isneginf(lm[b, ns:])) and np.all(np.isneginf(total[b, ns:])) and np.all(np.isfinite(total[b, :ns]))
        ref_lm, ref_tot = case["lm"][b][o][:ns], case["total"][b][o][:ns]
        tol_lm = RC.tolerance(case["e32"], ref_lm)
        tol_tot = abs(lw) * tol_lm + RC.FLOOR * np.maximum(1.0, np.abs(ref_tot))
        e_lm, e_tot = np.abs(lm[b, :ns] - ref_lm), np.abs(total[b, :ns] - ref_tot)
        assert np.all(e_lm <= tol_lm) and np.all(e_tot <= tol_tot), (label, b, (e_lm / tol_lm).max(), (e_tot / tol_tot).max())


@pytest.mark.parametrize("name", ALL)
def test_rescore_nbest(name, fp32_mode):
    case = RC.make(name)
    m = model(case["V"])
    ids, lengths, am, prefix = on_gpu(case)
    aw, lw, lb = case["weights"]

    def run():
        return m.rescore_nbest(ids, lengths, am, prefix=prefix, lm_weight=lw, am_weight=aw, length_bonus=lb, **_kwargs(case))

    got = run()
    check_ranked(case, got, name)
    again = run()                                                       # the same bits every run
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_static_max_nodes_inside_a_capture(fp32_mode):
    """max_nodes = int: nothing waits for the host, so the call records into a graph; the replay gives the eager bits and the overflow rule
    of the restatement"""
    case = RC.make("overflow")
    m = model(case["V"])
    ids, lengths, am, prefix = on_gpu(case)
    aw, lw, lb = case["weights"]

    def step():
        return m.rescore_nbest(ids, lengths, am, prefix=prefix, lm_weight=lw, am_weight=aw, length_bonus=lb, **_kwargs(case))

    eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    check_ranked(case, out, "overflow graph")
    assert [int((case["tries"][b]["leaf"] < 0).sum()) for b in range(2)] == [1, 1]


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def test_model_decode_and_franky(fp32_mode):
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainEncoder, BrainFormerCTC, Franky
    V = 307
    gpt = model(V)
    enc = bf.MAEConfig(window_size=200, n_electrodes=64, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512, n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=8, output_dim=V + 1, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)
    torch.manual_seed(3)
    m = BrainFormerCTC(cfg).cuda()                                      # the blank is class V: outside the LM's vocabulary
    with torch.no_grad():
        m.perceiver["to_words"].weight.normal_(0.0, 0.5)
    x = torch.randn(2, 200, 64, device="cuda")
    W, k = 6, 3
    kw = dict(lm_weight=0.4, length_bonus=0.2, eos_token_id=V - 1, bos_token_id=V - 1)
    ids, lengths, scores = m.decode(x, beam_width=W, nbest=W)
    want = gpt.rescore_nbest(ids, lengths, scores, **kw)
    got = m.decode(x, beam_width=W, nbest=k, lm=gpt, **kw)
    assert len(got) == 3 and got[0].shape == (2, k, 8)
    assert torch.equal(got[0], want[0][:, :k]) and torch.equal(got[1], want[1][:, :k]) and torch.equal(got[2], want[4][:, :k])
    best = m.decode(x, beam_width=W, lm=gpt, **kw)
    assert len(best) == 2 and torch.equal(best[0], want[0][:, 0]) and torch.equal(best[1], want[1][:, 0])
    assert int(want[6].min()) >= 1 and bool(torch.isfinite(want[4][:, 0]).all())
    # without lm: today's results, bit for bit
    logits = m.features(x)
    for a, b in zip(m.decode(x, beam_width=W, nbest=W), E.ctc_beam_decode(logits, blank=m.blank, beam_width=W, nbest=W, pad=-100)):
        assert torch.equal(a, b)
    for a, b in zip(m.decode(x, beam_width=W), [t[:, 0] for t in E.ctc_beam_decode(logits, blank=m.blank, beam_width=W, nbest=1, pad=-100)[:2]]):
        assert torch.equal(a, b)
    for a, b in zip(m.decode(x), E.ctc_greedy_decode(logits, blank=m.blank, pad=-100)):
        assert torch.equal(a, b)
    # Franky: the brain features are the prefix
    bcfg = bf.Config(encoder=enc, n_output_tokens=4, output_dim=128, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)
    torch.manual_seed(4)
    franky = Franky(BrainEncoder(bcfg).cuda(), gpt)
    got = franky.rescore(x, ids, lengths, scores, **kw)
    want = gpt.rescore_nbest(ids, lengths, scores, prefix=franky.brain_model(x), **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    plain = gpt.rescore_nbest(ids, lengths, scores, **kw)
    assert not torch.equal(got[3], plain[3])                            # the prefix reaches the scores
