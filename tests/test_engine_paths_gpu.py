"""The hand-written autograd Functions of frankenstein_amd/engine.py (AttnBranch, CrossAttnBranch, MlpBranch, NormLinear, LayerNormFn,
PatchEmbed, MaskedPatchEmbed, AssembleDecoder, GatherRows, ExpandQueries, Dropout, with the wgrad / norm_bwd helpers that accumulate into
a gradient arena) against the float64 restatement of tests/engine_ref.py, on every path of tests/engine_cases.py.

Each case: the engine's own host-side path queries are asked first and compared with the names in the case id; the Function then runs
with a recorder around the engine.K entry points and the kernels called must be the ones those names stand for; the output, the
input gradient(s) and every parameter gradient are compared with the reference on every element; the inputs must be unchanged.
Arena cases preload the flat gradient buffer with g0 (engine_ref.g0_pattern) and check grad - g0, a second forward / backward without
zeroing (g0 + 2 ref), that the Function handed autograd None for the parameters it accumulated itself, and that every parameter's
post-accumulate-grad hook fired once per backward; their side-stream twins meet the same bound after a device synchronize.

Bound per tensor, den = |ref| + rms(ref):
    fp32 mode  |got - ref| <= 1e-3 |ref| + 2e-5                       (the project's fp32 gradient bound, check_full_grads)
    bf16 mode  |got - ref| <= MARGIN * max(model_err / den) * den     MARGIN = 4, model_err the error of the CPU rounding model of
                                                                      engine_ref.py on the same case and tensor
tests/test_engine_paths_cpu.py shows that every planted bookkeeping defect exceeds twice this bound on every case it applies to.
A parameter gradient (kept in fp32) counts at least one fp32 unit roundoff, 2^-24, as its relative model error: a column sum of a few
bf16 values can be exact in the model's order of adding and inexact in the kernel's.
Prints "FRAC <function> <tensor> <paths> <largest error / bound>", <paths> being the path names of the case and its compute dtype.

FRAC maxima on the MI355X (every case passes), largest over the tensors of the cases that name the path:
  bf16  AttnBranch       rope_ps 0.47  rope 0.38  ident_ps 0.35  plain 0.37  inverse RoPE fused 0.47
        wgrad            tensors 0.46  adjacent 0.47  split_add 0.39  swiglu_slab 0.25  swiglu_add 0.25  side stream 0.47 (the same bits)
        norm_bwd         arena 0.47  tensors 0.46
        MlpBranch        swiglu_fused 0.42  swiglu 0.25  gelu 0.25  one_launch 0.25  dswiglu 0.42  plain 0.25
        CrossAttnBranch 0.38  NormLinear 0.48  LayerNormFn 0.72 (dgamma)  PatchEmbed / MaskedPatchEmbed / AssembleDecoder /
        ExpandQueries / Dropout 0.25 (the model's own rounding: the same values)  GatherRows 0 (exact)
  fp32  AttnBranch       rope 0.46  plain 0.47    wgrad  tensors 0.47  adjacent 0.41  split_add 0.35  swiglu_slab 0.39  swiglu_add 0.38
        MlpBranch        swiglu_fused 0.63  swiglu 0.61  gelu 0.28  dswiglu 0.63  plain 0.61    norm_bwd  arena 0.39  tensors 0.63
        CrossAttnBranch 0.16  NormLinear 0.06  LayerNormFn 0.01  PatchEmbed 0.05  MaskedPatchEmbed 0.02  the rest below 0.01"""
import pytest
import torch

from oracle import ref_models as R
from tests import engine_cases as EC
from tests import engine_ref as ER

pytestmark = pytest.mark.gpu

RECORDED = ("gemm_nt_rope", "gemm_nt", "rope_", "gemm_nt_swiglu", "gemm_nt_dswiglu", "mlp_bwd_fused", "gemm_tn", "gemm_tn_swiglu_", "add2d_",
            "norm_bwd", "dropout")


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import frankenstein_amd as fa
    from frankenstein_amd import engine, kernels
    yield engine, kernels
    fa.set_compute_dtype("bf16")


def expected_calls(case):
    """(kernel, flag) -> count for one forward + backward, from the path names of the case"""
    p, kw, fn = case.paths, case.kw, case.fn
    exp = {}

    def add(k, n=1):
        if n:
            exp[k] = exp.get(k, 0) + n

    groups = ER.WGRAD_GROUPS.get(fn, {})
    names = ER.param_names(case)
    for g, path in p.get("wgrad", {}).items():
        members = [n for n in groups[g] if n in names] or ["qkvw"]
        if path in ("tensors", "swiglu_add", "split_add"):
            add(("gemm_tn", False))
        if path == "adjacent":
            add(("gemm_tn", True))
        if path == "swiglu_slab":
            add(("gemm_tn_swiglu_", None))
        if path == "swiglu_add":
            add(("add2d_", None), 2)
        if path == "split_add":
            add(("add2d_", None), len(members))
    if "norm_bwd" in p:
        add(("norm_bwd", p["norm_bwd"] == "arena"))
    if fn == "attn":
        rope_gemm = p["proj"] in ("rope_ps", "rope", "ident_ps")
        if rope_gemm:
            add(("gemm_nt_rope", p["proj"] != "rope"))             # flag: a pre-scaled query table is passed
        add(("gemm_nt", None), 3 if rope_gemm else 4)
        add(("dropout", None), 2 if kw["drop"] else 0)
    elif fn == "cross":
        add(("gemm_nt", None), 6)
    elif fn == "mlp":
        fused = p["mlp"] == "swiglu_fused"
        add(("gemm_nt_swiglu", None), int(fused))
        add(("gemm_nt_dswiglu", None), int(p["mlp_bwd"] == "dswiglu"))
        add(("mlp_bwd_fused", None), int(p["mlp_bwd"] == "one_launch"))
        add(("gemm_nt", None), (1 if fused else 2) + {"one_launch": 0, "dswiglu": 1, "plain": 2}[p["mlp_bwd"]])
        add(("dropout", None), 2 if kw["drop"] else 0)
    elif fn == "normlinear":
        add(("gemm_nt", None), 2)
        add(("gemm_tn", False))
    elif fn in ("patch", "mpatch"):
        add(("gemm_nt", None))
        add(("gemm_tn", False))
    elif fn == "dropout":
        add(("dropout", None), 2)
    return exp


def install_recorder(monkeypatch, K):
    calls = {}

    def wrap(name, fn):
        def rec(*a, **k):
            flag = None
            if name == "gemm_tn":
                flag = bool(k.get("accumulate", a[3] if len(a) > 3 else False))
            elif name == "norm_bwd":
                flag = bool(k.get("accumulate", False))
            elif name == "gemm_nt_rope":
                flag = k.get("q_table") is not None
                calls.setdefault("rope_T", []).append(a[4])
            calls[(name, flag)] = calls.get((name, flag), 0) + 1
            return fn(*a, **k)
        return rec

    for name in RECORDED:
        monkeypatch.setattr(K, name, wrap(name, getattr(K, name)))
    return calls


def record_backward(monkeypatch, cls):
    outs = []
    orig = cls.backward

    def backward(ctx, *g):
        r = orig(ctx, *g)
        outs.append(r)
        return r

    monkeypatch.setattr(cls, "backward", staticmethod(backward))
    return outs


def build(case, inp, E, K):
    """-> (Function class, call() -> y, leaves name -> tensor (inputs then parameters), names of apply's tensor arguments in order)"""
    kw, fn = case.kw, case.fn
    cdt = ER.CDT[case.dtype]
    dev = "cuda"
    names = ER.param_names(case)
    P = {n: torch.nn.Parameter(inp[n].to(dev)) for n in names}
    X = {n: inp[n].to(dev, cdt).requires_grad_(True) for n in ER.input_names(case)}
    g = lambda n: P.get(n)
    nkind = K.NORM_RMS if kw.get("norm") == "rms" else K.NORM_LAYER
    eps = ER.NORM_EPS.get(kw.get("norm", "ln"), 1e-5)
    words = torch.tensor([ER.DROP_SEED, ER.DROP_STEP], dtype=torch.int32, device=dev)
    if fn == "attn":
        B, N = kw["B"], kw["N"]
        mk = kw["mask"]
        if mk == "none":
            mask = K.NO_MASK
        elif mk == "block_causal":
            mask = K.Mask(K.MASK_BLOCK_CAUSAL, 8)
        elif mk == "dense":
            mask = K.Mask.from_dense(R.block_causal_mask(N, 8).to(dev), N, N)
        elif mk == "causal":
            mask = K.Mask(K.MASK_CAUSAL)
        else:
            mask = K.Mask.from_padding(torch.ones(B, N, dtype=torch.bool, device=dev), inp["k_valid"].to(dev))
        rope = E.Rope(inp["rope"].to(dev)) if kw["rope"] else None
        spec = (kw["H"], kw["D"], mask, rope, kw["residual"], eps, nkind)
        if kw["drop"]:
            spec = spec + ((kw["drop"], words, ER.DROP_SITES[0], ER.DROP_SITES[1]),)
        ws = [P["qkvw"]] if kw["gpt"] else [P["qw"], P["kw"], P["vw"]]
        order = ["x", "ln_w", "ln_b", "pw", "pb", "qkv_b", None] + (["qkvw"] if kw["gpt"] else ["qw", "kw", "vw"])
        return E.AttnBranch, (lambda: E.AttnBranch.apply(X["x"], g("ln_w"), g("ln_b"), P["pw"], g("pb"), g("qkv_b"), spec, *ws)), X, P, order
    if fn == "cross":
        spec = (kw["H"], kw["D"], K.NO_MASK, 1e-5)
        order = ["x", "context", "ln_w", "ln_b", "qw", "kw", "vw", "pw", None]
        return E.CrossAttnBranch, (lambda: E.CrossAttnBranch.apply(X["x"], X["context"], P["ln_w"], P["ln_b"], P["qw"], P["kw"], P["vw"], P["pw"], spec)), X, P, order
    if fn == "mlp":
        spec = (kw["residual"], eps, nkind)
        if kw["drop"]:
            spec = spec + ((kw["drop"], words, ER.DROP_SITES[0]),)
        order = ["x", "ln_w", "ln_b", "up_w", "up_b", "gate_w", "down_w", "down_b", None]
        return E.MlpBranch, (lambda: E.MlpBranch.apply(X["x"], g("ln_w"), g("ln_b"), P["up_w"], g("up_b"), g("gate_w"), P["down_w"], g("down_b"), spec)), X, P, order
    if fn == "normlinear":
        order = ["x", "ln_w", "ln_b", "w", "b", None, None]
        return E.NormLinear, (lambda: E.NormLinear.apply(X["x"], g("ln_w"), g("ln_b"), P["w"], g("b"), 1e-5, kw["out_fp32"])), X, P, order
    if fn == "layernorm":
        order = ["x", "w", "b", None, None]
        return E.LayerNormFn, (lambda: E.LayerNormFn.apply(X["x"], P["w"], g("b"), eps, nkind)), X, P, order
    if fn == "patch":
        data = inp["data"].to(dev)
        return E.PatchEmbed, (lambda: E.PatchEmbed.apply(data, P["emb_w"], P["emb_b"], P["space"], kw["P"])), X, P, None
    if fn == "mpatch":
        kp = (kw["P"] + 31) // 32 * 32
        tok_all = K.patchify(inp["data"].to(dev), kw["P"], kp, cdt).view(kw["B"], kw["nT"] * kw["C"], kp)
        um = inp["unmasked"].to(dev)
        return E.MaskedPatchEmbed, (lambda: E.MaskedPatchEmbed.apply(tok_all, P["emb_w"], P["emb_b"], P["space"], um, kw["P"])), X, P, None
    if fn == "assemble":
        um, mk = inp["unmasked"].to(dev), inp["masked"].to(dev)
        return E.AssembleDecoder, (lambda: E.AssembleDecoder.apply(X["tokens"], P["mask_token"], P["pos_table"], um, mk)), X, P, None
    if fn == "gather":
        idx = inp["idx"].to(dev)
        return E.GatherRows, (lambda: E.GatherRows.apply(X["src"], idx)), X, P, None
    if fn == "expand":
        return E.ExpandQueries, (lambda: E.ExpandQueries.apply(P["q"], kw["B"])), X, P, None
    if fn == "dropout":
        return E.Dropout, (lambda: E.Dropout.apply(X["x"], (kw["drop"], words, ER.DROP_SITES[0]))), X, P, None
    raise KeyError(fn)


def path_label(case):
    """the path names of a case, comma-separated: projection, inverse RoPE, MLP forward and backward, the wgrad paths, norm_<path>, then the compute dtype"""
    p = case.paths
    names = [p[k] for k in ("proj", "rope_bwd", "mlp", "mlp_bwd") if p.get(k)]
    names += sorted(set(p.get("wgrad", {}).values())) + (["norm_" + p["norm_bwd"]] if "norm_bwd" in p else [])
    return ",".join(names + (["stream"] if case.stream else []) + [case.dtype])


def compare(case, name, got, ref, bnd, scale=1.0):
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - scale * ref).abs()
    b = scale * bnd
    pos = b > 0
    frac = float((err[pos] / b[pos]).max()) if bool(pos.any()) else 0.0
    exact_ok = bool((err[~pos] == 0).all())
    print(f"FRAC {case.fn} {name}{'' if scale == 1.0 else 'x2'} {path_label(case)} {frac:.3f}")
    return [] if (frac <= 1.0 and exact_ok and bool(torch.isfinite(got).all())) else [(name, scale, frac)]


@pytest.mark.parametrize("case", EC.CASES, ids=[c.id for c in EC.CASES])
def test_function_matches_float64_on_its_path(case, mods, monkeypatch):
    E, K = mods
    assert ER.query_paths(case) == case.paths
    inp, ref, model, bnd = ER.case_data(case)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    prev_dtype, prev_stream = E.compute_dtype(), E.wgrad_stream()
    E.set_compute_dtype(ER.CDT[case.dtype])
    try:
        if case.stream:
            E.enable_wgrad_stream(True)
        cls, call, X, P, order = build(case, inp, E, K)
        before = {n: t.detach().clone() for n, t in list(X.items()) + list(P.items())}
        arena_names = ER.arena_params(case)
        g0 = None
        if case.arena:
            lay, total = ER.arena_layout(case, inp)
            g0 = ER.g0_pattern(total).cuda()
            flat = g0.clone()
            for n in case.arena:
                P[n].grad = flat[lay[n][0]:lay[n][0] + lay[n][1]].view(P[n].shape)
                P[n]._fk_arena = True
        fired = {n: 0 for n in P}
        for n, p in P.items():
            p.register_post_accumulate_grad_hook(lambda _p, n=n: fired.__setitem__(n, fired[n] + 1))
        bouts = record_backward(monkeypatch, cls)
        calls = install_recorder(monkeypatch, K)
        dy = inp["dy"].to("cuda", torch.float32 if case.kw.get("out_fp32") else ER.CDT[case.dtype])
        dy0 = dy.clone()

        y = call()
        y.backward(dy)
        torch.cuda.synchronize()

        # the kernels called are the ones the path names stand for
        rope_T = calls.pop("rope_T", [])
        assert calls == expected_calls(case), (calls, expected_calls(case))
        if case.paths.get("proj") in ("rope_ps", "rope"):
            assert rope_T == [case.kw["N"]]
        if case.paths.get("proj") == "ident_ps":
            assert rope_T == [8]

        def grad_of(n):
            t = X[n] if n in X else P[n]
            if case.arena and n in case.arena:
                return t.grad - g0[lay[n][0]:lay[n][0] + lay[n][1]].view(t.shape)
            return t.grad

        bad = compare(case, "y", y, ref["y"], bnd["y"])
        assert y.dtype == (torch.float32 if case.kw.get("out_fp32") else ER.CDT[case.dtype])
        for n in list(X) + list(P):
            assert grad_of(n) is not None, n
            bad += compare(case, "d" + n, grad_of(n), ref["d" + n], bnd["d" + n])
        for n, t in list(X.items()) + list(P.items()):
            assert torch.equal(t.detach(), before[n]), f"{n} was modified"
        assert torch.equal(dy, dy0), "dy was modified"
        assert all(v == 1 for v in fired.values()), fired

        if order is not None:
            (outs,) = bouts
            for n, o in zip(order, outs):
                if n is None or (n not in X and n not in P):
                    assert o is None, n
                elif n in arena_names:
                    assert o is None, f"{n}: accumulated into the arena AND handed to autograd"
                else:
                    assert o is not None, n
        if case.arena:
            # a second forward / backward without zeroing: everything is added once more
            call().backward(dy)
            torch.cuda.synchronize()
            for n in P:
                bad += compare(case, "d" + n, grad_of(n), ref["d" + n], bnd["d" + n], scale=2.0)
            assert all(v == 2 for v in fired.values()), fired
        assert not bad, bad
    finally:
        E._WGRAD_STREAM = prev_stream
        E.set_compute_dtype(prev_dtype)
