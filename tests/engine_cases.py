"""Case table of the engine-level tests (tests/test_engine_paths_cpu.py, tests/test_engine_paths_gpu.py): one entry per call of a
hand-written torch.autograd.Function of frankenstein_amd/engine.py, with the names of the paths that call must take (the answers of
engine.attn_proj_path / attn_bwd_rope_path / mlp_path / mlp_bwd_path / wgrad_path / norm_bwd_path).  Plain data: no torch, no GPU.

Case.kw holds the shapes and switches tests/engine_ref.py builds the inputs and the float64 reference from; Case.paths the expected
path names; Case.arena = (names of the parameters whose .grad are views of one flat fp32 buffer, in buffer order) for the cases that
accumulate straight into a gradient arena; Case.stream runs the case with the weight-gradient side stream enabled; Case.env the
environment switches set around the call."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

DTYPES = ("bf16", "fp32")

# paths no legal input reaches: (query, name, the check that bars it).  Not tested, not removed.
UNREACHABLE = (
    ("attn_proj_path", "plain_rope", "needs D % 8 != 0 or 3 H D % 8 != 0; fk_attn_fwd takes head_dim 8 / 16 / 32 / 64 / 128 only "
                                     "(csrc/attention.hip, the head_dim check of the attention entry points)"),
    ("attn_bwd_rope_path", "kernel", "needs D % 4 != 0: the same head_dim check of fk_attn_fwd, which runs first"),
)

# gemm_tn(da [M, 128], h [M, 128]) in bf16: the smallest M whose plan has more than one split (tests/test_engine_paths_cpu.py pins it
# against kernels.gemm_tn_route)
SLAB_ROWS = 257


@dataclass(frozen=True)
class Case:
    fn: str
    name: str
    dtype: str
    kw: dict
    paths: dict
    arena: Optional[Tuple[str, ...]] = None
    stream: bool = False
    env: dict = field(default_factory=dict)

    @property
    def id(self) -> str:
        names = [str(v) for k, v in sorted(self.paths.items()) if k not in ("wgrad", "norm_bwd") and v is not None]
        if self.arena is not None:
            names += sorted(set(self.paths.get("wgrad", {}).values())) + ["norm_" + self.paths["norm_bwd"]] * ("norm_bwd" in self.paths)
        return "-".join([self.fn, self.name, self.dtype] + names + (["stream"] if self.stream else []))


def _ps(dtype, D, mask, drop):
    return dtype == "bf16" and D == 64 and mask != "dense" and not drop


def attn_cases():
    out = []
    base = dict(B=2, N=72, H=2, D=64, d=128, rope="shared", cache=80, mask="block_causal", norm="ln", residual=True, gpt=False, drop=0.0)

    def add(name, env=None, ident=True, **over):
        kw = dict(base, **over)
        for dt in DTYPES:
            ps = _ps(dt, kw["D"], kw["mask"], kw["drop"])
            if kw["rope"]:
                proj, rb = ("rope_ps" if ps else "rope"), "fused"
            else:
                ok = ps and ident and kw["N"] >= 64 and (kw["B"] * kw["N"]) % 8 == 0
                proj, rb = ("ident_ps" if ok else "plain"), None
            paths = {"proj": proj, "rope_bwd": rb, "wgrad": {"pw": "tensors", "qkv": "tensors"}}
            if kw["norm"] != "none":
                paths["norm_bwd"] = "tensors"
            out.append(Case("attn", name, dt, kw, paths, env=env or {}))

    add("blockcausal")
    add("dense", mask="dense")
    add("h4d32", H=4, D=32)
    add("rope_per_sample", rope="per_sample")
    add("norope_keypad", rope=None, mask="keypad")
    add("norope_nomask", rope=None, mask="none")
    add("norope_n60", rope=None, mask="none", N=60)
    add("norope_b1n73", rope=None, mask="none", B=1, N=73)
    add("norope_env", rope=None, mask="none", env={"FK_ATTN_NO_IDENT_PRESCALE": "1"}, ident=False)
    add("gpt", rope=None, mask="causal", gpt=True)
    add("gpt_dropout", rope=None, mask="causal", gpt=True, drop=0.1)
    add("rms", norm="rms")
    add("nonorm", norm="none")
    add("nonorm_nores", norm="none", residual=False)
    add("nores", residual=False)
    return out


def cross_cases():
    out = []
    for T in (8, 70):
        for H, D in ((2, 64), (4, 16)):
            kw = dict(B=2, T=T, Nc=200, H=H, D=D, d=128)
            for dt in DTYPES:
                out.append(Case("cross", f"t{T}h{H}d{D}", dt, kw,
                                {"wgrad": {"pw": "tensors", "qw": "tensors", "kv": "tensors"}, "norm_bwd": "tensors"}))
    return out


def _mlp_paths(dt, kw):
    if kw["kind"] == "gelu":
        mp = "gelu"
    else:
        mp = "swiglu_fused" if (not kw["up_bias"] and kw["hidden"] % 8 == 0) else "swiglu"
    rows = kw["B"] * kw["N"]
    if mp != "swiglu_fused":
        bp = "plain"
    elif dt == "bf16" and kw["d"] == 384 and kw["hidden"] % 32 == 0 and rows >= 32768:
        bp = "one_launch"
    else:
        bp = "dswiglu"
    paths = {"mlp": mp, "mlp_bwd": bp, "wgrad": {"down": "tensors", "up": "tensors"}}
    if kw["norm"] != "none":
        paths["norm_bwd"] = "tensors"
    return paths


def mlp_cases():
    out = []
    base = dict(B=2, N=72, d=128, hidden=64, kind="swiglu", up_bias=False, down_bias=False, norm="ln", residual=True, drop=0.0)

    def add(name, dtypes=DTYPES, **over):
        kw = dict(base, **over)
        for dt in dtypes:
            out.append(Case("mlp", name, dt, kw, _mlp_paths(dt, kw)))

    add("swiglu")
    add("swiglu_h4", dtypes=("fp32",), hidden=4)         # K = hidden of the down projection: a multiple of 4 in fp32, of 8 in bf16
    add("swiglu_upbias", up_bias=True)                   # the unfused SwiGLU arm in bf16: an up bias (no model has one)
    add("gelu", kind="gelu", up_bias=True, down_bias=True)
    add("gelu_dropout", kind="gelu", up_bias=True, down_bias=True, drop=0.1)
    add("rms", norm="rms")
    add("nonorm", norm="none")
    add("nonorm_nores", norm="none", residual=False)
    add("one_launch", dtypes=("bf16",), B=1, N=32769, d=384, hidden=32)
    return out


def normlinear_cases():
    out = []
    base = dict(B=2, N=36, d=128, nout=16, ln=True, bias=True, out_fp32=False)

    def add(name, dtypes=DTYPES, **over):
        kw = dict(base, **over)
        for dt in dtypes:
            out.append(Case("normlinear", name, dt, kw, {"norm_bwd": "tensors"} if kw["ln"] else {}))

    add("ln_bias")
    add("plain", ln=False, bias=False)
    add("ln_nobias", bias=False)
    add("nout13", nout=13)
    add("out_fp32", dtypes=("bf16",), out_fp32=True)
    return out


def small_cases():
    out = []
    for dt in DTYPES:
        for kind in ("ln", "rms"):
            out.append(Case("layernorm", kind, dt, dict(B=2, N=36, d=128, norm=kind), {"norm_bwd": "tensors"}))
        for P in (4, 6):
            out.append(Case("patch", f"p{P}", dt, dict(B=3, nT=6, C=5, P=P, d=128), {}))
            out.append(Case("mpatch", f"p{P}", dt, dict(B=3, nT=6, C=5, P=P, d=128, n=11), {}))
        out.append(Case("assemble", "n11m19", dt, dict(B=3, n=11, m=19, d=128), {}))
        out.append(Case("gather", "n11", dt, dict(B=3, N=30, n=11, d=128), {}))
        out.append(Case("expand", "m8", dt, dict(B=3, M=8, d=128), {}))
        out.append(Case("dropout", "p01", dt, dict(B=2, N=72, d=128, drop=0.1), {}))
    return out


def arena_cases():
    """Parameters in `arena` carry _fk_arena and their .grad are consecutive views, in this order, of one flat fp32 buffer preloaded
    with engine_ref.g0_pattern; every other parameter is an ordinary leaf."""
    out = []
    mlp = dict(B=2, N=72, d=128, hidden=64, kind="swiglu", up_bias=False, down_bias=False, norm="ln", residual=True, drop=0.0)
    attn = dict(B=2, N=72, H=2, D=64, d=128, rope="shared", cache=80, mask="block_causal", norm="ln", residual=True, gpt=False, drop=0.0)
    for dt in DTYPES:
        rope = "rope_ps" if dt == "bf16" else "rope"
        for stream in (False, True):
            out.append(Case("mlp", "arena_slab", dt, dict(mlp, B=1, N=SLAB_ROWS), {
                "mlp": "swiglu_fused", "mlp_bwd": "dswiglu", "wgrad": {"down": "adjacent", "up": "swiglu_slab"}, "norm_bwd": "arena"},
                arena=("up_w", "gate_w", "down_w", "ln_w", "ln_b"), stream=stream))
            out.append(Case("mlp", "arena_add_beta_only", dt, dict(mlp, B=1), {          # 72 rows: one split in either dtype
                "mlp": "swiglu_fused", "mlp_bwd": "dswiglu", "wgrad": {"down": "adjacent", "up": "swiglu_add"}, "norm_bwd": "tensors"},
                arena=("gate_w", "up_w", "ln_b", "down_w"), stream=stream))
            out.append(Case("attn", "arena_adjacent_rms", dt, dict(attn, norm="rms"), {
                "proj": rope, "rope_bwd": "fused", "wgrad": {"pw": "adjacent", "qkv": "adjacent"}, "norm_bwd": "arena"},
                arena=("qw", "kw", "vw", "ln_w", "pw"), stream=stream))
            out.append(Case("attn", "arena_split", dt, attn, {
                "proj": rope, "rope_bwd": "fused", "wgrad": {"pw": "tensors", "qkv": "split_add"}, "norm_bwd": "arena"},
                arena=("vw", "qw", "ln_b", "kw", "ln_w"), stream=stream))
        out.append(Case("attn", "arena_one_outside", dt, attn, {
            "proj": rope, "rope_bwd": "fused", "wgrad": {"pw": "adjacent", "qkv": "tensors"}, "norm_bwd": "tensors"},
            arena=("qw", "kw", "pw", "ln_w")))
    return out


CASES = attn_cases() + cross_cases() + mlp_cases() + normlinear_cases() + small_cases() + arena_cases()
assert len({c.id for c in CASES}) == len(CASES)
