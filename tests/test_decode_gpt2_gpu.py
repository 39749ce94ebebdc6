"""Decoding at the reference's real decoder size on the MI355X: GPT-2 124M (d = 768, 12 layers, 12 heads, V = 50257, synthetic
weights, tied head) against tests/golden/gpt2_124m_generate.npz, which tests/golden/make_golden_decode.py wrote by running the
reference (greedy, 8 new tokens behind a 32-token brain prefix; the reference's top-1 / top-2 logit gap is >= 1e-3 at every step, so
its tokens are a fair target).  Every decode step here has B <= 16 rows and runs on fk_gemv_nt; the 33-row prefill stays on the MFMA GEMM."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import synth

pytestmark = pytest.mark.gpu

T_PREFIX, NEW = 32, 8


@pytest.fixture(scope="module")
def z(golden):
    return golden("gpt2_124m_generate")


@pytest.fixture(scope="module")
def model():
    from frankenstein_amd.models import gpt2_model as g2
    g = g2.GPT(g2.GPTConfig(block_size=1024, vocab_size=50257, n_layer=12, n_head=12, n_embd=768, dropout=0.0, bias=True))
    shapes = {k: tuple(v.shape) for k, v in g.state_dict().items() if v is not None}
    st = synth.make_state(shapes, synth.SEED_WEIGHTS, ("attn_mask",))
    for k in list(st):
        if k.endswith("lm_head.weight"):                       # tied: one tensor, generated under the wte key
            st[k] = st[k.replace("lm_head.weight", "transformer.wte.weight")]
    missing, unexpected = g.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    assert not missing and not unexpected
    return g.cuda().eval()


@pytest.fixture
def mode(request):
    fa.set_compute_dtype(request.param)
    yield request.param
    fa.set_compute_dtype("bf16")


def inputs(z, B=1):
    prefix = torch.from_numpy(synth.make_motion_targets(1, T_PREFIX, 768, seed=int(z["seed"]))).cuda()
    start = torch.from_numpy(z["start"]).cuda()
    return start.repeat(B, 1), prefix.repeat(B, 1, 1)


def new_cache(g, B, total):
    from frankenstein_amd import engine as E
    return [torch.zeros((B, total, 2 * g.config.n_embd), dtype=E.compute_dtype(), device="cuda") for _ in g.transformer.h]


def teacher_forced_logits(g, z, steps):
    """[steps, V] last-position logits of the cached path, fed the reference's tokens"""
    from frankenstein_amd.models.brainformer import _prep
    start, prefix = inputs(z)
    cache = new_cache(g, 1, T_PREFIX + 1 + NEW)
    toks = torch.from_numpy(z["tokens"]).cuda()
    logits, pos = g._cached_logits(start, cache, 0, _prep(prefix))
    out = [logits.float().cpu()[0]]
    for i in range(1, steps):
        logits, pos = g._cached_logits(toks[None, i:i + 1], cache, pos)
        out.append(logits.float().cpu()[0])
    return torch.stack(out)


@pytest.mark.parametrize("mode", ["fp32"], indirect=True)
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
def test_gpt2_124m_greedy_tokens_match_the_reference(model, z, mode, use_graph):
    start, prefix = inputs(z)
    out = model.generate(start.clone(), NEW, prefix=prefix, top_k=1, use_graph=use_graph)
    assert out.cpu().tolist() == z["tokens"].tolist()


@pytest.mark.parametrize("mode", ["fp32"], indirect=True)
def test_gpt2_124m_step_logits_match_the_reference(model, z, mode):
    """per-step logits of _cached_logits (step 0: the prefill, steps 1-7: fk_gemv_nt at M = 1) vs the stored columns 0::97, the 64
    largest values and the log-sum-exp, each within 1e-4 (the tolerance of the gpt2-nano decode test)"""
    lg = teacher_forced_logits(model, z, NEW).double()
    stride = int(z["col_stride"])
    top = torch.gather(lg, 1, torch.from_numpy(z["top_ids"]))
    errs = (float((lg[:, ::stride] - torch.from_numpy(z["cols"]).double()).abs().max()),
            float((top - torch.from_numpy(z["top_vals"]).double()).abs().max()),
            float((torch.logsumexp(lg, -1) - torch.from_numpy(z["lse"])).abs().max()))
    print("max |logit - reference|: columns %.3e, top-64 %.3e, log-sum-exp %.3e" % errs)
    assert max(errs) <= 1e-4, errs
    assert lg.argmax(-1).tolist() == z["tokens"][1:].tolist()


@pytest.mark.parametrize("mode", ["bf16"], indirect=True)
def test_gpt2_124m_bf16_graph_and_eager_agree(model, z, mode):
    start, prefix = inputs(z)
    eager = model.generate(start.clone(), NEW, prefix=prefix, top_k=1, use_graph=False)
    graph = model.generate(start.clone(), NEW, prefix=prefix, top_k=1, use_graph=True)
    assert eager.cpu().tolist() == graph.cpu().tolist()
    # step-0 logits within the project's bf16 bound of the reference: 2e-2 * max(1, |want| max) absolute, 2e-2 relative
    lg = teacher_forced_logits(model, z, 1)[0]
    stride = int(z["col_stride"])
    for got, want in ((lg[::stride], torch.from_numpy(z["cols"][0])), (lg[torch.from_numpy(z["top_ids"][0])], torch.from_numpy(z["top_vals"][0]))):
        print(f"bf16 step 0: max |logit - reference| = {float((got - want).abs().max()):.3e}, |want| max = {float(want.abs().max()):.3e}")
        torch.testing.assert_close(got, want, atol=2e-2 * max(1.0, float(want.abs().max())), rtol=2e-2)


@pytest.mark.parametrize("mode", ["fp32", "bf16"], indirect=True)
def test_gpt2_124m_batched_decode_is_the_single_sample_decode(model, z, mode):
    """B = 3 with the same prompt: the first sample's tokens are the B = 1 run's, and a decode step on three copies of one sample's caches
    (and on sixteen) gives each copy the B = 1 step's logits bit for bit (fk_gemv_nt's rows do not depend on the batch), host- and device-position step alike"""
    from frankenstein_amd.models.brainformer import _prep
    start, prefix = inputs(z)
    one = model.generate(start.clone(), NEW, prefix=prefix, top_k=1, use_graph=False)
    s3, p3 = inputs(z, 3)
    assert model.generate(s3.clone(), NEW, prefix=p3, top_k=1, use_graph=False).cpu().tolist() == one.cpu().tolist()
    assert model.generate(s3.clone(), NEW, prefix=p3, top_k=1, use_graph=True).cpu().tolist() == one.cpu().tolist()
    if mode == "fp32":
        assert one.cpu().tolist() == z["tokens"].tolist()
    total = T_PREFIX + 1 + 2
    c1 = new_cache(model, 1, total)
    l0, pos = model._cached_logits(start, c1, 0, _prep(prefix))
    tok = l0.argmax(-1)
    copies = {B: [c.repeat(B, 1, 1).contiguous() for c in c1] for B in (3, 16)}        # B = 16: the kernel's largest row bucket
    copies_dev = {B: [c.clone() for c in cs] for B, cs in copies.items()}
    l1, _ = model._cached_logits(tok[:, None].contiguous(), c1, pos)
    for B in (3, 16):
        lB, _ = model._cached_logits(tok.repeat(B)[:, None].contiguous(), copies[B], pos)
        lBd = model._decode_logits_dev(tok.repeat(B).contiguous(), copies_dev[B], torch.tensor([pos], dtype=torch.int32, device="cuda"))
        for b in range(B):
            assert torch.equal(lB[b], l1[0]), (B, b)
            assert torch.equal(copies[B][0][b], c1[0][0]) and torch.equal(copies_dev[B][0][b], c1[0][0]), (B, b)
            # behind the first layer the device-position step has gone through fk_attn_decode instead of fk_attn_fwd: its copies agree among themselves
            assert torch.equal(copies[B][-1][b], c1[-1][0]) and torch.equal(copies_dev[B][-1][b], copies_dev[B][-1][0]), (B, b)
            assert torch.equal(lBd[b], lBd[0]), (B, b)
