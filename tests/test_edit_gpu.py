"""Edit distance on the MI355X (csrc/editdist.hip) against the restatement tests/edit_ref.py on the cases of tests/edit_cases.py:
distances, pairwise tables and MBR ranking exactly (the risks within max(4 e32, 8 * 2^-24 * max(1, |risk|))), error rates against the host
metric on a tiny model's decodes, the MWER loss and its gradient against torch's float64 CPU composition, stream capture, and the model
surface.

The MWER tolerance is not fixed beforehand: the same composition is evaluated with torch in fp32 on the CPU, its error against float64 is
measured, and the device gets 4 x that, with the floor of tests/test_ctc_gpu.py, 8 * 2^-24 * max(1, max |nll|), for the cases where torch
happens to be exact (an nll carries a rounding of 2^-24 |nll|, and p = softmax(-nll) passes it on in full).  Both errors are printed (profiles/edit_distance.md records them)."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import _lib
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from frankenstein_amd.utils import metrics
from tests import edit_cases as EC
from tests import edit_ref as ER

pytestmark = pytest.mark.gpu

ROUTES = {"lane": _lib.EDIT_LANE, "lane_ref": _lib.EDIT_LANE, "lane_swap": _lib.EDIT_LANE, "lane_long": _lib.EDIT_LANE, "rows4": _lib.EDIT_ROWS4,
          "rows4_swap": _lib.EDIT_ROWS4, "rows16_min": _lib.EDIT_ROWS16, "rows16": _lib.EDIT_ROWS16, "big_ids": _lib.EDIT_LANE, "same": _lib.EDIT_LANE,
          "disjoint": _lib.EDIT_LANE, "clamp": _lib.EDIT_LANE}


def strided(view):
    """a case's view on the device with the garbage around it: the whole buffer is copied, the same slice is taken"""
    base = view._base.cuda()
    assert base.shape == view._base.shape
    return base[:, :view.shape[1], :view.shape[2]]


def dev(t):
    return None if t is None else t.cuda()


@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def capture(step):
    """step() once on a side stream, then inside a stream capture (which raises on anything that waits for the host) -> (graph, outputs)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    return graph, out


# ---- distances --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, explicit", [(n, e) for n in sorted(EC.DISTANCE) for e in (True, False) if e or n != "clamp"],
                         ids=lambda v: v if isinstance(v, str) else ("lengths" if v else "pad"))
def test_edit_distance(name, explicit):
    c = EC.make_distance(name, explicit)
    assert K.edit_distance_route(c.La, c.Lb) == ROUTES[name]
    a, b = strided(c.a), strided(c.b)
    assert a.stride(1) > c.La and b.stride(1) > c.Lb
    dist, alen = K.edit_distance(a, dev(c.alen), b, dev(c.blen), EC.PAD, want_lengths=True)
    assert dist.dtype == torch.int32 and alen.dtype == torch.int32
    assert np.array_equal(dist.cpu().numpy(), c.dist), (dist.cpu().numpy(), c.dist)
    assert np.array_equal(alen.cpu().numpy(), c.alen_ref)
    again = K.edit_distance(a, dev(c.alen), b, dev(c.blen), EC.PAD)
    assert torch.equal(again, dist)


def test_engine_edit_distance_forms():
    """[P, L] pairs, a reference [B, L] against [B, n, L] and list against list, lengths of the leading shape"""
    c = EC.make_distance("lane_ref", True)
    a, b = strided(c.a), strided(c.b)
    d = E.edit_distance(a[:, 0], b, c.alen[:, 0].cuda(), c.blen.cuda())
    assert d.shape == (5, 6) and np.array_equal(d.cpu().numpy(), c.dist)
    p = E.edit_distance(a[:, 0], b[:, 3], c.alen[:, 0].cuda(), c.blen[:, 3].cuda())
    assert p.shape == (5,) and np.array_equal(p.cpu().numpy(), c.dist[:, 3])
    c = EC.make_distance("lane", False)
    d = E.edit_distance(strided(c.a), strided(c.b))
    assert np.array_equal(d.cpu().numpy(), c.dist)
    e = E.edit_distance(torch.empty((2, 0), dtype=torch.int64, device="cuda"), torch.tensor([[3, 4, -100], [-100, 1, 1]], device="cuda"))
    assert e.tolist() == [2, 0]


# ---- pairwise distances and MBR ---------------------------------------------------------------------------------------------------------

def check_ranking(c, r, what):
    inp = c["inp"]
    B, n, T = c["B"], c["n"], c["T"]
    assert np.array_equal(r.dist.cpu().numpy(), c["dist"]), what
    assert np.array_equal(r.order.cpu().numpy(), c["order"]), (what, r.order.cpu().numpy(), c["order"])
    assert np.array_equal(r.n_valid.cpu().numpy(), c["n_valid"]), what
    ids, lengths, scores = inp.ids.numpy(), inp.lengths.numpy(), inp.scores.numpy()
    got_ids, got_len, got_sc, got_risk = (t.cpu().numpy() for t in (r.ids, r.lengths, r.scores, r.risk))
    for b in range(B):
        for k in range(n):
            h = c["order"][b, k]
            L = min(max(int(lengths[b, h]), 0), T)
            assert got_len[b, k] == L and np.array_equal(got_ids[b, k, :L], ids[b, h, :L]) and np.all(got_ids[b, k, L:] == EC.PAD), (what, b, k)
            assert got_sc[b, k] == scores[b, h] or (np.isnan(got_sc[b, k]) and np.isnan(scores[b, h]))
            want = c["risk"][b, h]
            if np.isfinite(want):
                assert abs(float(got_risk[b, k]) - want) <= c["tol"][b, h], (what, b, k, got_risk[b, k], want, c["tol"][b, h])
            else:
                assert got_risk[b, k] == np.inf


@pytest.mark.parametrize("name", sorted(EC.RANKING))
def test_mbr_rerank(name):
    c = EC.make_ranking(name)
    inp = c["inp"]
    ids, lengths, scores = strided(inp.ids), inp.lengths.cuda(), inp.scores.cuda()
    r = E.mbr_rerank(ids, lengths, scores, scale=c["scale"])
    check_ranking(c, r, name)
    risk_in, _ = K.mbr_rank(r.dist, ids, lengths, scores, c["scale"])
    want = c["risk"]
    fin = np.isfinite(want)
    got = risk_in.cpu().numpy()
    assert np.all(np.abs(got[fin] - want[fin]) <= c["tol"][fin]) and np.all(got[~fin] == np.inf)
    r2 = E.mbr_rerank(ids, lengths, scores, scale=c["scale"])
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(r, r2))


def test_pairwise_without_scores_holds_every_pair():
    c = EC.make_ranking("invalid")
    inp = c["inp"]
    got = K.nbest_pairwise_distance(strided(inp.ids), inp.lengths.cuda(), None).cpu().numpy()
    for b in range(c["B"]):
        want = ER.pairwise(inp.ids[b].tolist(), inp.lengths[b].numpy(), None)
        assert np.array_equal(got[b], want) and np.all(np.diag(got[b]) == 0) and got[b].min() >= 0


def test_mbr_rerank_in_a_graph():
    c = EC.make_ranking("r32")
    inp = c["inp"]
    ids, lengths, scores = strided(inp.ids), inp.lengths.cuda(), inp.scores.cuda()
    eager = E.mbr_rerank(ids, lengths, scores, scale=c["scale"])
    graph, out = capture(lambda: E.mbr_rerank(ids, lengths, scores, scale=c["scale"]))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, eager))
    check_ranking(c, out, "graph")


# ---- the model: error rates, the oracle, MBR decoding, the MWER weight -------------------------------------------------------------------

def small_model(**kw):
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    enc = bf.MAEConfig(window_size=200, n_electrodes=64, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512, n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=8, output_dim=6, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)
    torch.manual_seed(3)
    m = BrainFormerCTC(cfg, **kw).cuda()
    with torch.no_grad():                                 # a head that does not start at zero, so that the frames differ
        m.perceiver["to_words"].weight.normal_(0.0, 0.5)
    return m, torch.randn(4, 200, 64, device="cuda")


def small_targets():
    return torch.tensor([[1, 2, 3, -100, -100], [0, 0, 4, 1, 2], [3, -100, -100, -100, -100], [2, 2, 1, 0, -100]], device="cuda")


def test_error_rate_and_oracle_on_model_decodes(fp32_mode):
    m, x = small_model()
    tg = small_targets()
    refs = tg.tolist()
    for kw in (dict(), dict(beam_width=4, topk=3), dict(beam_width=4, topk=3, nbest=3)):
        out = m.decode(x, **kw)
        ids = out[0][:, 0] if out[0].dim() == 3 else out[0]
        rate, errors, ref_len = m.error_rate(x, tg, **kw)
        assert rate.device.type == "cuda" and rate.dim() == 0
        hyps = [ER.seq(r, None, -100) for r in ids.tolist()]
        assert errors.tolist() == [metrics.edit_distance(ER.seq(r, None, -100), h) for r, h in zip(refs, hyps)]
        assert ref_len.tolist() == [3, 5, 1, 4]
        assert abs(float(rate) - metrics.token_error_rate(refs, ids.tolist())) <= 2.0 ** -22
    ids, lengths, scores = m.decode(x, beam_width=4, topk=3, nbest=4)
    best, index = E.nbest_oracle(ids, lengths, scores, tg)
    for b in range(4):
        d = [metrics.edit_distance(ER.seq(refs[b], None, -100), ids[b, i, :int(lengths[b, i])].tolist()) if np.isfinite(float(scores[b, i])) else 1 << 40
             for i in range(4)]
        assert int(best[b]) == min(d) and int(index[b]) == d.index(min(d))


def _gpt(V):
    from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
    from tests import rescore_cases as RC
    cfg = RC.gpt_cfg(V)
    gpt = GPT(GPTConfig(block_size=cfg.block_size, vocab_size=V, n_layer=cfg.n_layer, n_head=cfg.n_head, n_embd=cfg.n_embd, bias=True)).cuda().eval()
    own = gpt.state_dict()
    with torch.no_grad():
        for k, v in RC.state_dict(V).items():
            own[k].copy_(v)
    E.bump_weight_epoch()
    return gpt


def test_model_decode_with_mbr(fp32_mode):
    """decode(mbr=True) is engine.mbr_rerank of the whole final list of the path asked for, with that path's ranking score; without mbr the
    results are today's bits"""
    from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
    m, x = small_model()
    lm = NGramLM.from_corpus(zipf_sequences(40, 6, m.blank, (2, 8), 5), 3, 6)
    gpt = _gpt(307)
    with torch.no_grad():
        logits = m.features(x)
    W, Kc, nbest = 4, 3, 2
    gkw = dict(lm_weight=0.7, length_bonus=0.2, eos_token_id=306, bos_token_id=306)

    def same(out, r):
        assert len(out) == 3 and out[0].shape == (4, nbest, 8)
        assert torch.equal(out[0], r.ids[:, :nbest]) and torch.equal(out[1], r.lengths[:, :nbest]) and torch.equal(out[2], -r.risk[:, :nbest])

    plain = E.ctc_beam_decode(logits, blank=m.blank, beam_width=W, topk=Kc, nbest=W, pad=-100)
    same(m.decode(x, beam_width=W, topk=Kc, nbest=nbest, mbr=True, mbr_scale=0.5), E.mbr_rerank(*plain, scale=0.5))
    best = m.decode(x, beam_width=W, topk=Kc, mbr=True, mbr_scale=0.5)
    r = E.mbr_rerank(*plain, scale=0.5)
    assert len(best) == 2 and torch.equal(best[0], r.ids[:, 0]) and torch.equal(best[1], r.lengths[:, 0])
    fused = E.ctc_beam_decode_lm(logits, lm, blank=m.blank, beam_width=W, topk=Kc, nbest=W, lm_weight=0.8, length_bonus=0.5)
    same(m.decode(x, beam_width=W, topk=Kc, nbest=nbest, ngram=lm, ngram_weight=0.8, ngram_bonus=0.5, mbr=True),
         E.mbr_rerank(fused[0], fused[1], fused[4]))
    res = gpt.rescore_nbest(plain[0], plain[1], plain[2], **gkw)
    same(m.decode(x, beam_width=W, topk=Kc, nbest=nbest, lm=gpt, mbr=True, mbr_scale=2.0, **gkw), E.mbr_rerank(res[0], res[1], res[4], scale=2.0))
    with pytest.raises(ValueError, match="beam_width"):
        m.decode(x, mbr=True)
    # without mbr: the existing engine calls, bit for bit
    want = E.ctc_beam_decode(logits, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, pad=-100)
    assert all(torch.equal(a, b) for a, b in zip(m.decode(x, beam_width=W, topk=Kc, nbest=nbest), want))
    want = E.ctc_greedy_decode(logits, blank=m.blank, pad=-100)
    assert all(torch.equal(a, b) for a, b in zip(m.decode(x), want))
    got = m.decode(x, beam_width=W, topk=Kc, nbest=nbest, ngram=lm, ngram_weight=0.8, ngram_bonus=0.5)
    want = E.ctc_beam_decode_lm(logits, lm, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, lm_weight=0.8, length_bonus=0.5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[4])
    got = m.decode(x, beam_width=W, topk=Kc, nbest=nbest, lm=gpt, **gkw)
    assert torch.equal(got[0], res[0][:, :nbest]) and torch.equal(got[1], res[1][:, :nbest]) and torch.equal(got[2], res[4][:, :nbest])


def test_model_forward_with_and_without_mwer(fp32_mode):
    m, x = small_model()
    tg = small_targets()
    assert m.mwer_weight is None
    loss, logits = m(x, tg)
    want = E.ctc_loss(logits.detach(), tg, blank=m.blank, reduction="mean", zero_infinity=True, pad_value=-100)
    assert torch.equal(loss.detach(), want)
    m.mwer_weight, m.mwer_beam, m.mwer_nbest = 0.5, 4, 3
    loss2, logits2 = m(x, tg)
    assert torch.equal(logits2, logits)
    mw = E.ctc_mwer_loss(logits.detach(), tg, beam_width=4, nbest=3, blank=m.blank)
    assert torch.equal(loss2.detach(), want + 0.5 * mw) and bool(torch.isfinite(loss2))
    loss2.backward()
    g = m.perceiver["to_words"].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    m2, _ = small_model(mwer_weight=0.5, mwer_beam=4, mwer_nbest=3)
    assert torch.equal(m2(x, tg)[0].detach(), loss2.detach())


# ---- the MWER loss ------------------------------------------------------------------------------------------------------------------------

def mwer_refs(name, nbest, ce_weight):
    c = EC.make_mwer(name, nbest)
    args = (c.targets, c.target_lengths.numpy(), c.ids, c.lengths.numpy(), c.scores.numpy(), c.blank)
    loss64, grad64, nll, errors, valid = ER.mwer(c.logits, *args, ce_weight=ce_weight)
    loss32, grad32, *_ = ER.mwer(c.logits, *args, ce_weight=ce_weight, dtype=torch.float32)
    err_loss = abs(loss32 - loss64)
    err_grad = float((grad32.double() - grad64).abs().max())
    scale = max(1.0, float(np.abs(nll[np.isfinite(nll)]).max()) if np.isfinite(nll).any() else 1.0)
    return c, loss64, grad64, valid, (err_loss, err_grad), max(4.0 * err_loss, EC.FLOOR * scale), max(4.0 * err_grad, EC.FLOOR * scale)


@pytest.mark.parametrize("ce_weight", [0.0, 0.3], ids=["mwer", "mwer+ce"])
@pytest.mark.parametrize("nbest", [1, 4])
@pytest.mark.parametrize("name", sorted(EC.MWER))
def test_ctc_mwer_loss(name, nbest, ce_weight):
    c, loss64, grad64, valid, errs, tol_loss, tol_grad = mwer_refs(name, nbest, ce_weight)
    leaf = c.logits.cuda().requires_grad_(True)
    hyps = (c.ids.cuda(), c.lengths.cuda(), c.scores.cuda())
    tg, tl = c.targets.cuda(), c.target_lengths.cuda()
    loss = E.ctc_mwer_loss(leaf, tg, nbest=nbest, blank=c.blank, ce_weight=ce_weight, hyps=hyps, target_lengths=tl)
    loss.backward()
    got_loss, got_grad = float(loss), leaf.grad.cpu().double()
    d_loss, d_grad = abs(got_loss - loss64), float((got_grad - grad64).abs().max())
    print(f"\nmwer {name} nbest={nbest} ce={ce_weight}: torch fp32 CPU error loss {errs[0]:.3e} grad {errs[1]:.3e}; device error loss {d_loss:.3e} "
          f"grad {d_grad:.3e}; allowed {tol_loss:.3e} / {tol_grad:.3e}")
    assert bool(torch.isfinite(leaf.grad).all()) and np.isfinite(got_loss)
    assert d_loss <= tol_loss and d_grad <= tol_grad
    if ce_weight == 0.0:
        if nbest == 1:
            assert got_loss == 0.0 and float(leaf.grad.abs().max()) == 0.0
        for b in range(valid.shape[0]):
            if not valid[b].any():                                      # a sentence without a valid hypothesis: no term, no gradient, no NaN
                assert float(leaf.grad[b].abs().max()) == 0.0
    else:
        leaf.grad = None
        parts = E.ctc_mwer_loss(leaf, tg, nbest=nbest, blank=c.blank, hyps=hyps, target_lengths=tl) + \
            ce_weight * E.ctc_loss(leaf, tg, None, tl, blank=c.blank)
        assert torch.equal(parts.detach(), loss.detach())               # the documented sum
    again = E.ctc_mwer_loss(leaf.detach(), tg, nbest=nbest, blank=c.blank, ce_weight=ce_weight, hyps=hyps, target_lengths=tl)
    assert torch.equal(again, loss.detach())


def test_ctc_mwer_loss_searches_its_own_list():
    """hyps=None: the list is ctc_beam_decode on the detached logits"""
    c = EC.make_mwer("small", 4)
    lg, tg, tl = c.logits.cuda(), c.targets.cuda(), c.target_lengths.cuda()
    hyps = E.ctc_beam_decode(lg, blank=0, beam_width=6, topk=3, nbest=4)
    want = E.ctc_mwer_loss(lg, tg, blank=0, hyps=hyps, target_lengths=tl)
    got = E.ctc_mwer_loss(lg, tg, beam_width=6, nbest=4, topk=3, blank=0, target_lengths=tl)
    assert torch.equal(got, want) and bool(torch.isfinite(got))


def test_ctc_mwer_loss_in_a_graph():
    """forward and backward inside a stream capture; the replay gives the eager bits"""
    c = EC.make_mwer("small", 4)
    leaf = c.logits.cuda().requires_grad_(True)
    tg, tl = c.targets.cuda(), c.target_lengths.cuda()

    def step():
        loss = E.ctc_mwer_loss(leaf, tg, beam_width=6, nbest=4, topk=3, blank=0, ce_weight=0.2, target_lengths=tl)
        loss.backward()
        return loss.detach()

    loss0 = step()
    grad0 = leaf.grad.clone()
    leaf.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    leaf.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss1 = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss0) and torch.equal(leaf.grad, grad0) and bool(torch.isfinite(grad0).all())


def test_mwer_combine_kernel():
    """fk_mwer_combine alone against the restatement: validity by nll, score and length, coefficients = d loss / d nll, the count"""
    nll = torch.tensor([[0.7, 1.4, 1.4, 7.0], [float("inf"), 2.0, 0.5, 1.0], [1.0, 1.0, 1.0, 1.0]])
    errors = torch.tensor([[0, 2, 4, 9], [1, 3, 0, 2], [5, 5, 5, 5]], dtype=torch.int32)
    scores = torch.tensor([[-1.0, -2.0, -3.0, float("-inf")], [-1.0, -2.0, -3.0, -4.0], [float("-inf")] * 4])
    lengths = torch.tensor([[1, 2, 3, 4], [1, 2, 300, 4], [1, 1, 1, 1]])
    loss, coef, count, valid = K.mwer_combine(nll.cuda(), errors.cuda(), scores.cuda(), lengths.cuda(), 255)
    want_valid = torch.tensor([[1, 1, 1, 0], [0, 1, 0, 1], [0, 0, 0, 0]], dtype=torch.uint8)
    assert torch.equal(valid.cpu(), want_valid) and float(count) == 2.0
    for b in range(3):
        x = nll[b].double().clone().requires_grad_(True)
        v = want_valid[b].bool().tolist()
        if any(v):
            ref = ER.mwer_combine(x, errors[b].tolist(), v)
            ref.backward()
            assert abs(float(loss[b]) - float(ref)) <= 8 * 2.0 ** -24 * 9
            assert float((coef[b].cpu().double() - torch.where(want_valid[b].bool(), x.grad, torch.zeros(4, dtype=torch.float64))).abs().max()) <= 8 * 2.0 ** -24 * 9
        else:
            assert float(loss[b]) == 0.0 and float(coef[b].abs().max()) == 0.0
