"""LoRA through the model surface (GPT.add_lora / merge_lora, engine.AttnBranchLora / MlpBranchLora, the frozen-parameter rules of the
backward, merged shadows for inference, FusedAdamW / GraphedTrainStep / data parallel on the adapters alone), on a two-layer GPT with
n_embd = 128, two heads of 64, a 32-row prefix and 25 tokens at B = 2.

Tolerances are those of tests/test_models_gpu.py: fp32 mode test_gpt_small_fp32 (loss 1e-5, logits atol 1e-4, prefix gradient rtol 1e-3 /
atol 1e-6, parameter gradients rtol 1e-3 / atol 2e-5), bf16 mode test_bf16_drift_small (loss 3e-2, outputs 0.15, finite gradients);
the AdamW trajectory is compared as tests/test_train_gpu.py compares the full model (rtol 1e-3, atol 5e-5) and graph against eager as
test_graphed_train_step_is_bit_identical_to_eager does (bit for bit)."""
import numpy as np
import pytest
import torch

from oracle import ref_models as R

pytestmark = pytest.mark.gpu

B, T_PRE, T_TOK, D_EMB, VOCAB = 2, 32, 25, 128, 211


@pytest.fixture(autouse=True)
def _dtype():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import frankenstein_amd as fa
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def mk_gpt(dropout=0.0, seed=0, block_size=64):
    from frankenstein_amd.models import gpt2_model as g2
    torch.manual_seed(seed)
    return g2.GPT(g2.GPTConfig(block_size=block_size, vocab_size=VOCAB, n_layer=2, n_head=2, n_embd=D_EMB, dropout=dropout, bias=True)).cuda()


def inputs(t_tok=T_TOK):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randn(B, T_PRE, D_EMB, generator=g) * 0.5
    tk = torch.randint(0, VOCAB - 1, (B, t_tok), generator=g)
    tk[0, -3:] = -100
    idx = tk.clone()
    idx[idx == -100] = VOCAB - 1
    return prefix, tk, idx


def randomize_adapters(g, seed=9, b_std=0.05):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in g.lora_state_dict().items():
            p.copy_((torch.randn(p.shape, generator=gen) * (b_std if k.endswith("lora_B") else 0.1)).cuda())
    from frankenstein_amd import engine as E
    E.bump_weight_epoch()


def run(g, prefix, tk, idx):
    pf = prefix.cuda().requires_grad_(True)
    loss, logits = g(idx.cuda(), prefix=pf, targets=tk.cuda())
    loss.backward()
    return loss.detach(), logits.detach(), pf.grad


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_fresh_adapters_change_nothing(mode, dropout):
    import frankenstein_amd as fa
    from frankenstein_amd import engine as E
    fa.set_compute_dtype(mode)
    prefix, tk, idx = inputs()
    g = mk_gpt(dropout)
    g.train(dropout > 0)
    words = E.dropout_words(torch.device("cuda", torch.cuda.current_device()))
    torch.manual_seed(77)
    g(idx.cuda(), prefix=prefix.cuda(), targets=tk.cuda())                       # settles the seed words
    w0 = words.clone()
    base = run(g, prefix, tk, idx)
    start = idx[:, :4].cuda()
    g.eval()
    t0 = g.generate(start, 6, prefix=prefix.cuda(), top_k=1)
    g.train(dropout > 0)
    g.add_lora(rank=8, alpha=16.0)
    words.copy_(w0)                                                                # the same masks
    got = run(g, prefix, tk, idx)
    for a, b, what in zip(base, got, ("loss", "logits", "prefix gradient")):
        assert torch.equal(a, b), (what, float((a.float() - b.float()).abs().max()))
    g.eval()
    assert torch.equal(t0, g.generate(start, 6, prefix=prefix.cuda(), top_k=1))     # greedy, through the merged shadows
    g.merge_lora()
    assert torch.equal(t0, g.generate(start, 6, prefix=prefix.cuda(), top_k=1))


def reference(g, prefix, tk, idx):
    """float64 on the CPU: the oracle's GPT on W + s B A with the adapters as autograd leaves"""
    cfgo = R.gpt_config(block_size=64, vocab_size=VOCAB, n_layer=2, n_head=2, n_embd=D_EMB, dropout=0.0, bias=True)
    sd = {k: v.detach().double().cpu() for k, v in g.state_dict().items() if "lora_" not in k and k != "lm_head.weight"}
    leaves = {k: v.detach().double().cpu().requires_grad_(True) for k, v in g.lora_state_dict().items()}
    s = g.lora_config()["alpha"] / g.lora_config()["rank"]
    for k in [k for k in leaves if k.endswith("lora_A")]:
        w = k[:-len("lora_A")] + "weight"
        sd[w] = sd[w] + s * (leaves[k[:-1] + "B"] @ leaves[k])
    pr = prefix.double().requires_grad_(True)
    loss, logits = R.gpt_forward(sd, idx, pr, tk, cfgo)
    loss.backward()
    return loss.detach(), logits.detach(), pr.grad, {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("t_tok", [T_TOK, 40], ids=["25tok", "40tok-72rows"])
def test_nonzero_adapters_against_float64(t_tok):
    """fp32 mode at test_gpt_small_fp32's tolerances, bf16 mode at the bf16 drift bounds; 40 tokens make 72 rows per sample, which in
    bf16 takes the pre-scaled-query projection (engine.attn_proj_path "ident_ps"): the correction carries the query scale"""
    import frankenstein_amd as fa
    from frankenstein_amd import engine as E
    prefix, tk, idx = inputs(t_tok)
    g = mk_gpt(block_size=64 if t_tok == T_TOK else 128).add_lora(rank=8, alpha=16.0)
    randomize_adapters(g)
    rl, rlog, rpg, rgrads = reference(g, prefix, tk, idx)
    loss, logits, pg = run(g, prefix, tk, idx)
    assert abs(float(loss) - float(rl)) < 1e-5
    np.testing.assert_allclose(logits.float().cpu().numpy(), rlog.numpy(), atol=1e-4)
    np.testing.assert_allclose(pg.cpu().numpy(), rpg.numpy(), rtol=1e-3, atol=1e-6)
    named = dict(g.named_parameters())
    for k, want in rgrads.items():
        np.testing.assert_allclose(named[k].grad.cpu().numpy(), want.numpy(), rtol=1e-3, atol=2e-5, err_msg=k)
    assert all(p.grad is None for n, p in named.items() if "lora_" not in n)
    fa.set_compute_dtype("bf16")
    if t_tok == 40:
        assert E.attn_proj_path(B, T_PRE + t_tok, 2, 64, False, 1, False) == "ident_ps"
    for p in g.parameters():
        p.grad = None
    loss, logits, pg = run(g, prefix, tk, idx)
    assert abs(float(loss) - float(rl)) < 3e-2 and float((logits.float().cpu() - rlog).abs().max()) < 0.15
    assert all(torch.isfinite(named[k].grad).all() for k in rgrads) and torch.isfinite(pg).all()


def record(K, monkeypatch, fn):
    """the entry points fn launches, in order; the lazy (re)packing of weight shadows is left out: it depends on what ran before"""
    calls, real = [], K.call
    monkeypatch.setattr(K, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    try:
        fn()
    finally:
        monkeypatch.undo()
    return [c for c in calls if not c.startswith("fk_cast_pack")]


# loss backward of the two-layer GPT with a prefix, fp32 mode, everything trainable, no arena: recorded on the MI355X with the Python of
# the commit before adapters existed (head: CE, the zero-padded d-logits, dh, dw, LayerNorm; per block the MLP, then the attention)
_BLOCK_BWD = ["fk_gemm_tn", "fk_colsum", "fk_gemm_nt", "fk_gelu_bwd", "fk_gemm_nt", "fk_gemm_tn", "fk_colsum", "fk_norm_bwd",                 # MLP
              "fk_gemm_nt", "fk_gemm_tn", "fk_colsum", "fk_attn_bwd", "fk_gemm_nt", "fk_gemm_tn", "fk_colsum", "fk_norm_bwd"]                 # attention
PARENT_BACKWARD = (["fk_ce_loss_bwd", "fk_copy2d", "fk_gemm_nt", "fk_gemm_tn", "fk_norm_bwd"] + _BLOCK_BWD * 2 +
                   ["fk_copy2d", "fk_gpt_embed_bwd_wte", "fk_colsum"])


def test_frozen_base_does_no_weight_gradient_work(monkeypatch):
    from frankenstein_amd import kernels as K
    prefix, tk, idx = inputs()
    # nothing frozen, no adapters: the launch sequence the code had before adapters existed
    g = mk_gpt()
    pf = prefix.cuda().requires_grad_(True)
    loss, _ = g(idx.cuda(), prefix=pf, targets=tk.cuda())
    calls = record(K, monkeypatch, loss.backward)
    print("BACKWARD", calls)
    assert calls == PARENT_BACKWARD
    full_pg = pf.grad.clone()
    # a decoder frozen without adapters trains whatever feeds the prefix: the same prefix gradient, bit for bit, and no weight work
    for p in g.parameters():
        p.requires_grad_(False)
        p.grad = None
    pf = prefix.cuda().requires_grad_(True)
    loss, _ = g(idx.cuda(), prefix=pf, targets=tk.cuda())
    calls = record(K, monkeypatch, loss.backward)
    assert torch.equal(pf.grad, full_pg)
    assert not {"fk_gemm_tn", "fk_gpt_embed_bwd_wte", "fk_colsum", "fk_lora_wgrad"} & set(calls), calls
    assert all(p.grad is None for p in g.parameters())
    # adapted: one fk_lora_wgrad and one data-gradient fk_lora_fwd per adapted Linear, still none of the base products
    g.add_lora(rank=8)
    randomize_adapters(g)
    pf = prefix.cuda().requires_grad_(True)
    fwd = record(K, monkeypatch, lambda: globals().__setitem__("_loss", g(idx.cuda(), prefix=pf, targets=tk.cuda())[0]))
    assert fwd.count("fk_lora_fwd") == 8
    calls = record(K, monkeypatch, globals()["_loss"].backward)
    assert calls.count("fk_lora_wgrad") == 8 and calls.count("fk_lora_fwd") == 8
    assert not {"fk_gemm_tn", "fk_gpt_embed_bwd_wte", "fk_colsum"} & set(calls), calls
    assert all((p.grad is None) == ("lora_" not in n) for n, p in g.named_parameters())
    # the fused head loss: no [V, d] product either
    g.fuse_head_loss = True
    pf = prefix.cuda().requires_grad_(True)
    loss, _ = g(idx.cuda(), prefix=pf, targets=tk.cuda())
    calls = record(K, monkeypatch, loss.backward)
    assert "fk_transpose2d" not in calls and calls.count("fk_gemm_nt") == 2 * 4, calls      # per block: do, dh (attention), dg, dh (MLP); no head dw


def tiny_franky(seed=0):
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainEncoder, Franky
    torch.manual_seed(seed)
    enc = bf.MAEConfig(window_size=100, n_electrodes=16, patch_size=25, dim=64, n_layers=1, head_dim=32, hidden_dim=128, n_heads=2, n_kv_heads=2)
    cfg = bf.Config(encoder=enc, n_output_tokens=T_PRE, output_dim=D_EMB, dim=64, n_layers=1, head_dim=32, hidden_dim=128, n_heads=2, n_kv_heads=2)
    brain = BrainEncoder(cfg)
    fr = Franky(brain, mk_gpt(seed=seed + 1).cpu()).cuda()
    return fr


def franky_batches(n=3):
    g = torch.Generator().manual_seed(21)
    return [(torch.randn(B, 100, 16, generator=g).cuda(), torch.randint(0, VOCAB - 1, (B, T_TOK), generator=g).cuda(), None) for _ in range(n)]


def test_three_train_steps_on_an_adapted_franky():
    """brain model and adapters train, the GPT's base does not move; the adapters follow AdamW in float64 on the gradients of the
    float64 reference evaluated at the trajectory's own points (the brain features of each step enter as data)"""
    from frankenstein_amd.utils import train_utils as tu
    fr = tiny_franky()
    gpt = fr.llm_model
    gpt.add_lora(rank=8, alpha=16.0)
    randomize_adapters(gpt, b_std=0.02)
    for p in fr.brain_model.parameters():                                          # the adapters alone: the reference below needs no encoder
        p.requires_grad_(False)
    base = {k: v.detach().clone() for k, v in gpt.state_dict().items() if "lora_" not in k}
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3)
    opt = gpt.configure_optimizers(0.1, 1e-3, (0.9, 0.999), "cuda")
    trainable = [p for p in fr.parameters() if p.requires_grad]
    assert [id(p) for p in opt.arena.params] == [id(p) for p in trainable] and len(trainable) == 16
    assert opt.arena.numel == sum((p.numel() + 3) // 4 * 4 for p in trainable) and opt.m.numel() == opt.arena.numel
    assert all(p.grad is None for n, p in gpt.named_parameters() if "lora_" not in n)
    # float64 AdamW as configure_optimizers builds it: adapters undecayed, no clip, betas (0.9, 0.999), eps 1e-8
    assert opt.grad_clip is None and all(g["weight_decay"] == 0.0 for g in opt.param_groups if g["params"])
    w = {k: v.detach().double().cpu() for k, v in gpt.lora_state_dict().items()}
    m = {k: torch.zeros_like(v) for k, v in w.items()}
    v2 = {k: torch.zeros_like(v) for k, v in w.items()}
    for step, (x, tok, _) in enumerate(franky_batches()):
        with torch.no_grad():
            feats = fr.brain_model(x).float().cpu()
        _, _, _, grads = reference(_Shim(gpt, w), feats, tok.cpu(), tok.cpu())     # the reference at the float64 trajectory's own point
        tu.train_step(fr, (x, tok, None), opt, step, cfg)
        t = step + 1
        for k in w:
            gk = grads[k]
            m[k] = 0.9 * m[k] + 0.1 * gk
            v2[k] = 0.999 * v2[k] + 0.001 * gk * gk
            w[k] = w[k] - 1e-3 * (m[k] / (1 - 0.9 ** t)) / ((v2[k] / (1 - 0.999 ** t)).sqrt() + 1e-8)
    for k, p in gpt.lora_state_dict().items():
        np.testing.assert_allclose(p.float().cpu().numpy(), w[k].numpy(), rtol=1e-3, atol=5e-5, err_msg=k)
    for k, v in gpt.state_dict().items():
        if "lora_" not in k:
            assert torch.equal(v, base[k]), k                                      # the base masters are bit-unchanged
    assert float(opt.arena.grad.abs().max()) == 0.0


class _Shim:
    """what reference() reads of a GPT, with the adapters replaced by the float64 trajectory's"""

    def __init__(self, gpt, w):
        self.gpt, self.w = gpt, w

    def state_dict(self):
        return self.gpt.state_dict()

    def lora_state_dict(self):
        return self.w

    def lora_config(self):
        return self.gpt.lora_config()


def test_graphed_train_step_reproduces_eager_on_an_adapted_franky():
    import frankenstein_amd as fa
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("bf16")
    batches = franky_batches(4)
    tc = tu.TrainConfig(mixed_precision=True, use_scheduler=True, learning_rate=1e-3, warmup_iters=2, max_steps=10, lr_decay_iters=10)
    runs = []
    for graphed in (False, True):
        fr = tiny_franky()
        fr.llm_model.add_lora(rank=16, alpha=16.0)
        randomize_adapters(fr.llm_model, b_std=0.02)
        opt = tu.FusedAdamW(fr, lr=1e-3, weight_decay=1e-2, grad_clip=1.0, param_groups=tu.decay_groups(fr, 1e-2))
        if graphed:
            step = tu.GraphedTrainStep(fr, batches[0], opt, tc)
            losses = [float(step(b, i)) for i, b in enumerate(batches)]
        else:
            losses = [float(tu.train_step(fr, b, opt, i, tc)) for i, b in enumerate(batches)]
        runs.append((losses, opt.arena.flat.detach().clone(), opt.m.clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])




def step_logits(model, start, pfx):
    """final logits of the cached decode path after the prefix and the prompt (every Linear through _step_linear)"""
    from frankenstein_amd import engine as E
    from frankenstein_amd.models.brainformer import _prep
    d = model.config.n_embd
    cache = [torch.zeros(start.shape[0], model.config.block_size, 2 * d, dtype=E.compute_dtype(), device="cuda") for _ in model.transformer.h]
    with torch.no_grad():
        logits, _ = model._cached_logits(start, cache, 0, _prep(pfx))
    return logits.float().clone()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_inference_paths_read_merged_shadows(mode):
    import frankenstein_amd as fa
    from frankenstein_amd.models import gpt2_model as g2
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype(mode)
    prefix, tk, idx = inputs()
    pfx, start = prefix.cuda(), idx[:, :4].cuda()
    g = mk_gpt().add_lora(rank=8, alpha=16.0)
    randomize_adapters(g)
    g.eval()

    def decode(model):
        return (model.generate(start, 8, prefix=pfx, top_k=1, use_graph=False), model.generate(start, 8, prefix=pfx, top_k=1, use_graph=True),
                model.generate_beam_search(start[:1], 6, pfx[:1], beam_width=3, topk=6, use_cache=True, seeds=[123]), step_logits(model, start, pfx))

    # a captured decode-step Linear: the graph keeps reading the merged shadow's storage
    lin = g.transformer.h[1].mlp.c_fc
    from frankenstein_amd import engine as E
    xs = torch.randn(2, D_EMB, device="cuda").to(E.compute_dtype())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        g2._step_linear(xs, lin)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ys = g2._step_linear(xs, lin)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    before = ys.clone()
    with torch.no_grad():
        assert torch.equal(before, g2._step_linear(xs, lin))
    # a further optimizer step
    g.train()
    opt = tu.FusedAdamW(g, lr=5e-2, weight_decay=0.0)
    lin = g.transformer.h[1].mlp.c_fc
    with torch.no_grad():                                                          # the arena moved the adapters: capture again on the new masters
        with torch.cuda.stream(side):
            g2._step_linear(xs, lin)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ys = g2._step_linear(xs, lin)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    assert torch.equal(ys, before)
    loss, _ = g(idx.cuda(), prefix=pfx, targets=tk.cuda())
    loss.backward()
    opt.step()
    g.eval()
    graph.replay()                                                                 # no re-capture: refresh_shadows refilled the storage in place
    with torch.no_grad():
        eager = g2._step_linear(xs, lin)
    assert torch.equal(ys, eager) and not torch.equal(ys, before)
    live = decode(g)
    assert not torch.equal(live[3], torch.zeros_like(live[3]))
    g.merge_lora()
    merged = decode(g)
    for a, b, what in zip(live, merged, ("generate", "generate (graph)", "beam search", "logits")):
        assert torch.equal(a, b), what
    assert list(g.state_dict()) == list(mk_gpt().state_dict()) and g.lora_config() is None


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import frankenstein_amd as fa
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("fp32")
    fr = tiny_franky()
    fr.llm_model.add_lora(rank=8, alpha=16.0)
    randomize_adapters(fr.llm_model, seed=9 + rank, b_std=0.02)                    # replicas that did not start identical: rank 0's are taken
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3)
    opt = tu.FusedAdamW(fr, lr=1e-3, weight_decay=0.0, bucket_bytes=64 << 10)
    sent, real = [], dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (sent.append(t.numel() * t.element_size()), real(t, *a, **k))[1]
    for step, (x, tok, _) in enumerate(franky_batches(2)):
        xb, tb, _ = tu.shard_batch((x, tok, None), rank, world)
        tu.train_step(fr, (xb, tb, None), opt, step, cfg)
    torch.cuda.synchronize()
    trainable = [p for p in fr.parameters() if p.requires_grad]
    out[rank] = dict(adapters={k: v.cpu().numpy() for k, v in fr.llm_model.lora_state_dict().items()}, sent=sum(sent),
                     arena_bytes=opt.arena.numel * 4, want_bytes=4 * sum((p.numel() + 3) // 4 * 4 for p in trainable),
                     frozen_in_arena=sum(1 for p in opt.arena.params if not p.requires_grad),
                     base_bytes=4 * sum(p.numel() for n, p in fr.llm_model.named_parameters() if "lora_" not in n))
    dist.destroy_process_group()


def test_data_parallel_exchanges_the_trainable_arena_only():
    import torch.multiprocessing as mp
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert len(out) == world
    for k, v in out[0]["adapters"].items():
        np.testing.assert_array_equal(v, out[1]["adapters"][k], err_msg=k)         # both ranks end with identical adapters
    for r in range(world):
        o = out[r]
        assert o["arena_bytes"] == o["want_bytes"] and o["frozen_in_arena"] == 0
        assert o["sent"] == 2 * o["arena_bytes"], o                                # two steps, each all-reduces the trainable arena once
        assert o["arena_bytes"] < o["base_bytes"]                                   # and not the GPT's base
