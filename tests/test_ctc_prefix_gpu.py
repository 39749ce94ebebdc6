"""Joint CTC / attention decoding on the MI355X: fk_ctc_prefix_init / fk_ctc_prefix_score against the float64 restatement
(tests/ctc_prefix_ref.py) on the cases of tests/ctc_prefix_cases.py, a whole search without a model through the select and backtrack
kernels, and GPT.generate_beam_search / Franky.generate_beam with the ctc_* arguments.

Tolerances.  A joint value is compared with float64 within 4 x the error of the same restatement run in float32 on that case (measured
here, never from the kernel's output), not below one fp32 ulp of the case's largest |psi|; floor entries and rows of finished beams are
compared bit for bit with the float32 restatement (their three roundings are exact statements).  States likewise, one bound per case,
with the largest magnitude among the states and the logits in place of |psi| (_state_check says why).  Decisions (parents, tokens) are compared exactly where the restatement's margins are >= 1e-3, which
tests/test_ctc_prefix_cpu.py asserts for the listed salts.  The measured figures: profiles/ctc_joint_decode.md."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa  # noqa: F401
from tests import cases as C
from tests import ctc_prefix_cases as CC
from tests import ctc_prefix_ref as R
from tests.test_beam_batched_gpu import three_sentences
from tests.test_beam_gpu import TMAX, K, build_franky, fp32_mode, i32, select_ref, small_gpt  # noqa: F401
from tests.test_kernels_gpu import dev

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
NAN = float("nan")


def _ulp32(x):
    return float(np.spacing(f32(max(abs(float(x)), 1e-30))))


def _logits_tensor(logits, dtype, pad):
    """[S, T, C] on the device in `dtype`, each frame followed by `pad` columns of NaN the kernels must not read"""
    S, T, Cn = logits.shape
    buf = torch.full((S, T, Cn + pad), NAN, dtype=torch.float32)
    buf[..., :Cn] = torch.from_numpy(logits)
    return buf.to(torch.bfloat16 if dtype == "bf16" else torch.float32).cuda()[..., :Cn]


def _plant(cs, buf, hyps, W):
    """the hypotheses (one Hyps of W rows per sentence) into state buffer `buf`; everything else of the state is NaN / -7"""
    for t in cs.st:
        t.fill_(NAN)
    cs.psi.fill_(NAN)
    cs.last.fill_(-7)
    for g, h in enumerate(hyps):
        Tg = h.r_n.shape[1]
        sl = slice(g * W, g * W + W)
        cs.st[buf][sl, 0, :Tg] = torch.from_numpy(h.r_n.astype(f32)).cuda()
        cs.st[buf][sl, 1, :Tg] = torch.from_numpy(h.r_b.astype(f32)).cuda()
        cs.psi[buf, sl] = torch.from_numpy(h.psi.astype(f32)).cuda()
        cs.last[buf, sl] = torch.from_numpy(h.last.astype(np.int32)).cuda()


def _state_check(cs, buf, rows, W, T, want, want32, what, scale=0.0):
    """the state rows `rows` of buffer `buf` against the float64 hypotheses `want` (per sentence): -inf where float64 has -inf and behind the
    sentence's frames, last exact, values within one bound for the whole case: 4 x the float32 restatement's own largest error on these
    rows, not below one fp32 ulp of the largest magnitude involved (the states, and `scale`, the largest |logit|: every entry is a sum of
    y = logit - row_lse terms, which carry the rounding of their operands however small the sum comes out)"""
    st, psi, last = cs.st[buf].cpu().numpy(), cs.psi[buf].cpu().numpy(), cs.last[buf].cpu().numpy()
    parts = []
    for r in rows:
        g, b = divmod(r, W)
        h, h32 = want[g], want32[g]
        Tg = h.r_n.shape[1]
        assert int(last[r]) == int(h.last[b]), (what, r)
        assert np.all(st[r, :, Tg:] == -np.inf), (what, r)
        for got, w64, w32 in ((st[r, 0, :Tg], h.r_n[b], h32.r_n[b]), (st[r, 1, :Tg], h.r_b[b], h32.r_b[b]), (psi[r:r + 1], h.psi[b:b + 1], h32.psi[b:b + 1])):
            fin = np.isfinite(w64)
            assert np.array_equal(np.isfinite(got), fin) and np.all(got[~fin] == -np.inf), (what, r)
            parts.append((got[fin].astype(f64), w64[fin], w32[fin].astype(f64)))
    got, w64, w32 = (np.concatenate([p[i] for p in parts]) if parts else np.zeros(0) for i in range(3))
    if not len(got):
        return 0.0, 0.0
    bound = max(4 * float(np.abs(w32 - w64).max()), _ulp32(max(float(np.abs(w64).max()), scale)))
    err = float(np.abs(got - w64).max())
    assert err <= bound, (what, err, bound)
    return err, bound


# =============================================================================================== 1. one step from planted states
@pytest.mark.parametrize("c", CC.ONE_STEP, ids=CC.one_id)
def test_one_step_from_planted_states_against_float64(K, c):  # noqa: F811
    e = CC.one_step(c)
    S, W, k, T = c.S, c.W, c.k, c.T
    logits = _logits_tensor(e["logits"], c.dtype, c.pad)
    assert logits.stride(1) == c.C + c.pad
    lens = None if c.lengths is None else torch.tensor(e["lens"], dtype=torch.int64, device="cuda")
    cs = K.ctc_prefix_init(logits, W, c.weight, e["blank"], lens)
    par = c.step & 1
    src = par ^ 1 if e["advance"] else par
    _plant(cs, src, e["old"], W)
    st = K.BeamState("cuda", W, c.step + 1, TMAX, seed=list(range(S)), groups=S, eos=c.eos if c.eos >= 0 else None)
    st.step.fill_(c.step)
    st.parent_log.fill_(-5)
    st.tok_log.fill_(-5)
    if e["advance"]:
        st.parent_log[c.step - 1] = torch.from_numpy(e["parent"]).cuda()
        st.tok_log[c.step - 1] = torch.from_numpy(e["tok"]).cuda()
    if c.eos >= 0:
        st.fin.copy_(torch.from_numpy(e["fin"]))
    before = [t.clone() for t in cs.st] + [cs.psi.clone(), cs.last.clone()]
    top_lp, top_id = dev(torch.from_numpy(e["top_lp"])).clone(), dev(torch.from_numpy(e["top_id"]))
    K.ctc_prefix_score_(top_lp, top_id, cs, st, broadcast=c.broadcast)
    got = top_lp.cpu().numpy()
    floor, want, want32 = e["floor"], e["want"], e["want32"]
    rows_fin = [q for q in range(got.shape[0]) if e["fin"][q * W if c.broadcast else q]]
    assert np.array_equal(got[rows_fin].view(np.uint32), e["top_lp"][rows_fin].view(np.uint32))                # finished rows: untouched
    assert np.array_equal(got[floor].view(np.uint32), want32[floor].view(np.uint32))                           # floor entries: exact
    err = float(np.abs(got.astype(f64) - want)[~floor].max(initial=0.0))
    print(f"{CC.one_id(c)}: max |joint - float64| = {err:.3g}, bound {e['tol']:.3g} (float32 restatement {e['err32']:.3g}, largest |psi| {e['psi_max']:.4g})")
    assert np.isfinite(got).all() and err <= e["tol"]
    # the state: the buffer the step read is as planted; the other one holds the new hypotheses of the live rows and nothing else
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(cs.st[src], before[src]) and same(cs.psi[src], before[2][src]) and same(cs.last[src], before[3][src])
    if e["advance"]:
        live = [r for r in range(S * W) if e["live"][r]]
        dead = [r for r in range(S * W) if not e["live"][r]]
        serr, sbound = _state_check(cs, par, live, W, T, e["new"], e["new32"], CC.one_id(c), float(np.abs(e["logits"]).max()))
        print(f"    state: max |state - float64| = {serr:.3g}, bound {sbound:.3g}")
        assert bool(torch.isnan(cs.st[par][dead]).all()) and bool((cs.last[par][dead] == -7).all())
    else:
        assert same(cs.st[par ^ 1], before[par ^ 1])
    assert int(st.step) == c.step and bool((st.parent_log[c.step:] == -5).all())


def test_a_step_outside_the_logs_writes_nothing(K):  # noqa: F811
    e = CC.one_step(CC.ONE_STEP[5])
    c = e["case"]
    cs = K.ctc_prefix_init(_logits_tensor(e["logits"], c.dtype, 0), c.W, c.weight, e["blank"])
    st = K.BeamState("cuda", c.W, 2, TMAX, seed=[1], groups=c.S, eos=c.eos)
    top_id = dev(torch.from_numpy(e["top_id"]))
    for step in (-1, 3):
        _plant(cs, 0, e["old"], c.W)
        before = [t.clone() for t in cs.st]
        st.step.fill_(step)
        top_lp = dev(torch.from_numpy(e["top_lp"])).clone()
        K.ctc_prefix_score_(top_lp, top_id, cs, st)
        assert torch.equal(top_lp.cpu(), torch.from_numpy(e["top_lp"]))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(cs.st, before))


@pytest.mark.parametrize("dtype,pad,lens", [("f32", 0, None), ("bf16", 5, (33, 0, 17))])
def test_init_is_the_empty_hypothesis_advanced_by_the_prompt(K, dtype, pad, lens):  # noqa: F811
    rng = np.random.default_rng(7)
    S, W, T, Cn, blank = 3, 4, 33, 41, 40
    logits = (rng.standard_normal((S, T, Cn)) * 3).astype(f32)
    if dtype == "bf16":
        logits = CC.bf16_round(logits)
    prompt = np.array([[3, 3], [8, 40], [5, 6]], np.int64)                     # a repeated label; a blank among the labels (impossible); two labels
    Tg = [T] * S if lens is None else list(lens)
    for P in (0, 2):
        cs = K.ctc_prefix_init(_logits_tensor(logits, dtype, pad), W, 0.3, blank, None if lens is None else torch.tensor(Tg, device="cuda"),
                               torch.from_numpy(prompt[:, :P]).cuda() if P else None)
        want = {dt: [R.Hyps.cat([R.hyp_of(R.log_softmax_rows(logits[g, :Tg[g]], dt), blank, prompt[g, :P].tolist())] * W) for g in range(S)] for dt in (f64, f32)}
        lse = np.stack([np.log(np.exp(logits[g].astype(f64)).sum(-1)) for g in range(S)])
        assert float(np.abs(cs.row_lse.cpu().numpy() - lse).max()) <= 1e-5
        err, bound = _state_check(cs, 0, range(S * W), W, T, want[f64], want[f32], f"init P={P}", float(np.abs(logits).max()))
        print(f"init {dtype} P={P}: max |state - float64| = {err:.3g}, bound {bound:.3g}")


# =============================================================================================== 2. a whole search without a model
@pytest.mark.parametrize("c", CC.LOOPS, ids=lambda c: f"T{c.T}")
def test_search_without_a_model_follows_the_restatement(K, c):  # noqa: F811
    """flat attention rows, peaked CTC frames: score -> select -> ... -> backtrack.  Every step's joint values, parents, tokens, scores and
    the states of the surviving hypotheses (so the states follow the parents across the two buffers) against the restatement; the best
    beam is what the greedy CTC decoder reads off the same frames"""
    from frankenstein_amd import engine as E
    e = CC.loop(c)
    assert e["margin"] >= 1e-3
    W, k, T = c.W, c.k, c.T
    logits = dev(torch.from_numpy(e["logits"]))[None]
    n = len(e["steps"])
    cs = K.ctc_prefix_init(logits, W, c.weight, e["blank"])
    st = K.BeamState("cuda", W, n, TMAX, seed=[CC.LOOP_SEED], groups=1, eos=CC.LOOP_EOS)
    cur, pos = torch.empty(W, dtype=torch.int64, device="cuda"), i32(-1)
    tol_sum = 0.0
    for s, want in enumerate(e["steps"]):
        bc = s == 0
        top_lp, top_id = dev(torch.from_numpy(want["top_lp"])).clone(), dev(torch.from_numpy(want["top_id"]))
        K.ctc_prefix_score_(top_lp, top_id, cs, st, broadcast=bc)
        got = top_lp.cpu().numpy()
        live = [q for q in range(got.shape[0]) if not want["fin_in"][q]]
        if live:
            psi = np.concatenate([np.abs(want["hyp"].psi[np.isfinite(want["hyp"].psi)]), [0.0]]).max()
            w = f64(f32(c.weight))
            d = (want["want"] - (1 - w) * want["top_lp"]) / w
            tol = max(4 * float(np.abs(want["want32"].astype(f64) - want["want"])[live].max()),
                      _ulp32(max(psi, np.abs(want["hyp"].psi[:len(got), None] + d)[live].max())))
            err = float(np.abs(got.astype(f64) - want["want"])[live].max())
            tol_sum += tol
            print(f"T={T} step {s}: max |joint - float64| = {err:.3g}, bound {tol:.3g}")
            assert err <= tol and not want["floor"][live].any()
        dead = [q for q in range(got.shape[0]) if want["fin_in"][q]]
        assert np.array_equal(got[dead], want["top_lp"][dead])
        if s > 0:
            _state_check(cs, s & 1, live, W, T, [want["hyp"]], [want["hyp32"]], f"T={T} step {s}", float(np.abs(e["logits"]).max()))
        K.beam_select_eos(top_lp, top_id, st, cur, pos, broadcast=bc)
        assert cur.cpu().tolist() == want["cur"] and st.parent_log[s].cpu().tolist() == want["parent"], s
        assert np.array_equal(st.fin.cpu().numpy(), want["fin"]), s
        serr = float(np.abs(st.scores.cpu().numpy().astype(f64) - want["scores"]).max())
        assert serr <= tol_sum + (s + 1) * _ulp32(np.abs(want["scores"]).max()), (s, serr, tol_sum)
    ids = torch.zeros((1, W, n), dtype=torch.int64, device="cuda")
    scores, lens = K.beam_backtrack(st, ids, 0, -100)
    best = ids[0, 0, :int(lens[0, 0])].cpu().tolist()
    greedy, glen = E.ctc_greedy_decode(logits, blank=e["blank"])
    assert best == greedy[0, :int(glen[0])].cpu().tolist() + [CC.LOOP_EOS] == list(c.target) + [CC.LOOP_EOS]


# =============================================================================================== 3. the model
WM, NEWM, TCTC = 4, 5, 12
SEEDS_CTC = [1, 2, 3, 4, 5]          # of the CTC frames; the first whose oracle margins are all >= 1e-3 on the forward the test runs is used


def ctc_frames(seed, S, V):
    """[S, TCTC, V + 1] fp32 on the device, the blank last"""
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn((S, TCTC, V + 1), generator=g) * 2).cuda()


def joint_oracle(g, start, pf, frames, weight, from_prompt=0):
    """The re-forward search with the device rule for ONE sentence and topk == beam_width (every entry is drawn, so the candidate set does
    not depend on the draws): float64 log_softmax of the un-cached forward + topk, the float64 restatement's joint values, select_ref.
    -> beams, scores, the smallest decision margin as a multiple of 1e-3 (the top-k boundary of the attention term; neighbours among the
    W + 1 best distinct candidates)"""
    V1 = frames.shape[-1]
    y = R.log_softmax_rows(frames[0].cpu().numpy().astype(f64))
    blank = V1 - 1
    t0 = start.shape[1]
    hyp = R.Hyps.cat([R.hyp_of(y, blank, start[0, t0 - from_prompt:].cpu().tolist())] * WM)
    beams, scores, margin = [start[0].cpu().tolist()] * WM, np.zeros(WM, f32), np.inf
    no_table = np.zeros((WM, 1), np.int32)
    for t in range(NEWM):
        with torch.no_grad():
            _, logits = g(torch.tensor(beams, device="cuda"), prefix=pf.expand(WM, -1, -1).contiguous())
        lp, ids = torch.log_softmax(logits[:, -1, :].double().cpu(), -1).topk(WM + 1, -1)
        margin = min(margin, float((lp[:, WM - 1] - lp[:, WM]).min()) / 1e-3)
        top_lp, top_id = lp[:, :WM].float().numpy(), ids[:, :WM].numpy()
        jt, floor = R.score_rows([y], blank, [hyp], top_lp.astype(f64), top_id, weight, W=WM)
        jt = jt.astype(f32)
        parent, cur, new_scores, _, _, _, pick = select_ref(jt, top_id, t == 0, WM, scores, 12345, t, -1, no_table)
        drawn = sorted(((float(f32(scores[i] + jt[0 if t == 0 else i][j])), tuple(beams[i]) + (int(top_id[0 if t == 0 else i][j]),))
                        for i in range(WM) for j in pick[i]), key=lambda cd: -cd[0])
        gaps = [a[0] - b[0] for a, b in zip(drawn[:WM], drawn[1:WM + 1]) if a[1] != b[1]]
        margin = min(margin, (min(gaps) if gaps else np.inf) / 1e-3)
        hyp = R.extend(y, blank, hyp.take(parent), np.array(cur))
        beams, scores = [beams[p] + [cc] for p, cc in zip(parent, cur)], new_scores
    return beams, scores, margin


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
def test_weight_zero_is_the_search_without_the_arguments(golden, fp32_mode, S, use_graph):  # noqa: F811
    g, zz, start, pf, cfgo = small_gpt(golden)
    starts, pfs = (start, pf) if S == 1 else three_sentences()
    frames = ctc_frames(1, S, cfgo.vocab_size)
    seeds = [101, 202, 303][:S]
    runs = []
    for kw in ({}, dict(ctc_logits=frames, ctc_weight=0.0, ctc_from_prompt=1), dict(ctc_logits=None, ctc_weight=0.0)):
        out = g.generate_beam_search(starts.clone(), 6, pfs, topk=10, beam_width=WM, use_cache=True, use_graph=use_graph, seeds=seeds, **kw)
        runs.append((out.cpu().tolist(), g.last_beams, g.last_beam_scores))
    assert runs[0] == runs[1] == runs[2]                   # ids and score bits


@pytest.mark.parametrize("weight", [0.3, 1.0])
def test_joint_search_equals_the_host_oracle_and_the_re_forward_path(golden, fp32_mode, weight):  # noqa: F811
    """topk == beam_width: the cached search with the scorer equals the host oracle beam for beam, eager and as a hipGraph (bit-identical to
    each other), and the use_cache=False path, which applies the rule as torch ops, returns the same best beam"""
    g, zz, start, pf, cfgo = small_gpt(golden)
    for s in SEEDS_CTC:
        frames = ctc_frames(s, 1, cfgo.vocab_size)
        want_beams, want_scores, margin = joint_oracle(g, start, pf, frames, weight, from_prompt=1)
        print(f"weight {weight} frames {s}: smallest decision margin {margin:.3g} x 1e-3")
        if margin >= 1.0:
            break
    else:
        pytest.fail("none of the five seeds keeps every decision clear of rounding")
    runs = []
    kw = dict(ctc_logits=frames, ctc_weight=weight, ctc_from_prompt=1)
    for use_graph in (False, True):
        out = g.generate_beam_search(start.clone(), NEWM, pf, topk=WM, beam_width=WM, use_cache=True, use_graph=use_graph, seeds=[12345], **kw)
        runs.append((out.cpu().tolist(), g.last_beams, g.last_beam_scores))
        assert sorted(g.last_beams) == sorted(want_beams), use_graph
        order, want_order = sorted(range(WM), key=lambda b: g.last_beams[b]), sorted(range(WM), key=lambda b: want_beams[b])
        err = float(np.abs(np.array(g.last_beam_scores)[order] - want_scores[want_order]).max())
        print(f"graph={use_graph}: max |score - oracle| = {err:.3g} (scores {np.round(want_scores[want_order], 4).tolist()})")
        assert err <= NEWM * 1e-4 * 2                      # per step one log-probability and one CTC term, 1e-4 each (the project's fp32 logit tolerance)
        assert out.cpu().tolist() == g.last_beams[int(np.argmax(g.last_beam_scores))]
    assert runs[0] == runs[1]                              # graph replay equals eager, bit for bit
    best = want_beams[int(np.argmax(want_scores))]
    host = g.generate_beam_search(start.clone(), NEWM, pf, topk=WM, beam_width=WM, use_cache=False, **kw)
    assert host.cpu().tolist() == best == runs[0][0]
    # bf16 frames, an end-of-text id and three sentences run through the same launches, eager and captured alike
    starts, pfs = three_sentences()
    many = dict(ctc_logits=ctc_frames(s, 3, cfgo.vocab_size).bfloat16(), ctc_weight=weight, ctc_input_lengths=torch.tensor([TCTC, 0, 7]))
    outs = []
    for use_graph in (False, True):
        out = g.generate_beam_search(starts.clone(), 6, pfs, topk=10, beam_width=WM, use_cache=True, use_graph=use_graph, seeds=[7, 8, 9], eos_token_id=3, **many)
        outs.append((out.cpu().tolist(), g.last_beams, g.last_beam_scores))
        assert out.shape == (3, 10) and all(np.isfinite(x) for row in g.last_beam_scores for x in row)
    assert outs[0] == outs[1]


def test_outside_the_scorer_s_envelope_the_re_forward_path_runs(golden, fp32_mode):  # noqa: F811
    """1025 frames: the call takes the re-forward loop (which applies the rule as torch ops) and returns a well-formed sequence"""
    g, zz, start, pf, cfgo = small_gpt(golden)
    frames = torch.randn((1, 1025, cfgo.vocab_size + 1), generator=torch.Generator().manual_seed(3)).cuda()
    g.last_beams = None
    out = g.generate_beam_search(start.clone(), 3, pf, topk=6, beam_width=3, use_cache=True, ctc_logits=frames, ctc_weight=0.3)
    assert out.shape == (4 + 3,) and torch.equal(out[:4].cpu(), start[0].cpu()) and 0 <= int(out.min()) and int(out.max()) < cfgo.vocab_size
    assert len(g.last_beams) == 3 and len(g.last_beams[0]) == 7           # the joint re-forward loop reports its beams
    # two sentences: sentence by sentence, each with its own frames and length; with an end-of-text id the other re-forward loop
    starts, pfs = three_sentences()
    frames2 = torch.randn((2, 1025, cfgo.vocab_size + 1), generator=torch.Generator().manual_seed(4)).cuda()
    for kw in ({}, dict(eos_token_id=3)):
        out = g.generate_beam_search(starts[:2].clone(), 3, pfs[:2], topk=6, beam_width=3, use_cache=True, ctc_logits=frames2, ctc_weight=0.3,
                                     ctc_input_lengths=[40, 9], ctc_from_prompt=1, **kw)
        assert out.shape == (2, 7) and torch.equal(out[:, :4], starts[:2]) and 0 <= int(out.min()) and int(out.max()) < cfgo.vocab_size


def test_franky_generate_beam_with_a_ctc_head(fp32_mode):  # noqa: F811
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    fr, x, gcfg = build_franky()
    fr.eval()
    enc = fr.brain_model.config.encoder if hasattr(fr.brain_model, "config") else None
    if enc is None:
        bcfg = C.cfg1()[0]
        enc = bf.MAEConfig(window_size=bcfg.encoder.window_size, n_electrodes=256, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512,
                           n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=16, output_dim=gcfg.vocab_size + 1, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4,
                    n_kv_heads=4)
    torch.manual_seed(3)
    ctc = BrainFormerCTC(cfg).cuda().eval()
    with torch.no_grad():
        ctc.perceiver["to_words"].weight.normal_(0.0, 0.5)
    assert ctc.blank == gcfg.vocab_size
    torch.manual_seed(3)
    plain = fr.generate_beam(x[0].numpy(), max_new_tokens=7)
    plain_scores = list(fr.llm_model.last_beam_scores)
    torch.manual_seed(3)
    off = fr.generate_beam(x[0].numpy(), max_new_tokens=7, ctc=ctc, ctc_weight=0.0)
    assert torch.equal(plain, off) and fr.llm_model.last_beam_scores == plain_scores
    torch.manual_seed(3)
    one = fr.generate_beam(x[0].numpy(), max_new_tokens=7, ctc=ctc, ctc_weight=0.3)
    assert one.shape == (8,) and int(one[0]) == 50256 and 0 <= int(one.min()) and int(one.max()) < gcfg.vocab_size
    assert all(np.isfinite(s) for s in fr.llm_model.last_beam_scores) and fr.llm_model.last_beam_scores != plain_scores
    many = fr.generate_beam(x[:3].numpy(), max_new_tokens=7, ctc=ctc, ctc_weight=0.3, stop=True)
    assert many.shape == (3, 8) and bool((many[:, 0] == 50256).all()) and 0 <= int(many.min()) and int(many.max()) < gcfg.vocab_size
    with pytest.raises(ValueError, match="ctc_weight"):
        fr.generate_beam(x[0].numpy(), ctc=ctc, ctc_weight=1.5)
