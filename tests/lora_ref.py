"""Float64 restatement (numpy) of the low-rank adapter of csrc/lora.hip, and the CPU evaluation that rounds where the kernels round.

    u   = x A^T                              A [r, K], x [M, K]
    out = res + s * colscale * (u B^T)       B [N, r], colscale(n) = q_scale for n < q_cols, 1 elsewhere
    du  = dy B                               (unscaled: the kernel's transposed-role call stores this and scales the data gradient)
    dx  = s * du A
    dB  = s * dy^T u
    dA  = s * du^T x
    merged W' = W + s * B A

tests/test_lora_cpu.py pins these to torch.autograd in float64 (a derivation check).  `rounded_*` evaluate the same formulas in torch on
the CPU with the kernels' rounding points: operands in the compute dtype, fp32 accumulation, ONE rounding of u (and of du) and one of the
output; their error against the float64 result is the yardstick of the random-operand GPU tests (4 x its largest value)."""
import numpy as np
import torch

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def colscale(N, q_cols=0, q_scale=1.0):
    c = np.ones(N, dtype=np.float64)
    c[:q_cols] = q_scale
    return c


def forward(x, A, B, s, res=None, q_cols=0, q_scale=1.0):
    """(u [M, r], out [M, N]) in float64"""
    x, A, B = (np.asarray(v, dtype=np.float64) for v in (x, A, B))
    u = x @ A.T
    out = s * colscale(B.shape[0], q_cols, q_scale)[None, :] * (u @ B.T)
    if res is not None:
        out = out + np.asarray(res, dtype=np.float64)
    return u, out


def backward(x, A, B, s, dy, q_cols=0, q_scale=1.0):
    """(du, dx, dA, dB) in float64 for the upstream gradient dy of `out`; du is UNSCALED (dy_c B with dy_c = colscale * dy), dx is the
    term the adapter adds to the data gradient"""
    x, A, B, dy = (np.asarray(v, dtype=np.float64) for v in (x, A, B, dy))
    dyc = dy * colscale(B.shape[0], q_cols, q_scale)[None, :]
    u = x @ A.T
    du = dyc @ B
    dx = s * (du @ A)
    dB = s * (dyc.T @ u)
    dA = s * (du.T @ x)
    return du, dx, dA, dB


def merge(W, A, B, s):
    W, A, B = (np.asarray(v, dtype=np.float64) for v in (W, A, B))
    return W + s * (B @ A)


# ------------------------------------------------------------------------------------------------ the kernels' rounding points, on the CPU
def _t(v, dt):
    return torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dt)


def rounded_forward(x, A, B, s, dtype, res=None, q_cols=0, q_scale=1.0):
    """torch on the CPU: operands in the compute dtype, fp32 products / sums, u rounded once, out rounded once -> (u, out) as float64"""
    dt = TDT[dtype]
    xf, Af, Bf = (_t(v, dt).float() for v in (x, A, B))
    u = (xf @ Af.t()).to(dt)
    cs = torch.as_tensor(colscale(Bf.shape[0], q_cols, q_scale)).float() * np.float32(s)
    out = cs[None, :] * (u.float() @ Bf.t())
    if res is not None:
        out = out + _t(res, dt).float()
    return u.double().numpy(), out.to(dt).double().numpy()


def rounded_wgrad(dy, u, du, x, s, dtype):
    """(dA, dB) from compute-dtype operands with fp32 sums, as float64"""
    dt = TDT[dtype]
    dyf, uf, duf, xf = (_t(v, dt).float() for v in (dy, u, du, x))
    return (np.float32(s) * (duf.t() @ xf)).double().numpy(), (np.float32(s) * (dyf.t() @ uf)).double().numpy()


def rounded_merge(W, A, B, s):
    Wf, Af, Bf = (_t(v, torch.float32) for v in (W, A, B))
    return (Wf + np.float32(s) * (Bf @ Af)).double().numpy()


# ------------------------------------------------------------------------------------------------ exact operands
def exact_operands(M, N, K, r, seed, a_shift=-3, b_shift=-2):
    """Small-integer operands (float64 arrays holding values every compute dtype represents) with an asymmetric ramp in one column of
    each.  A is sparse (at most four non-zeros per row, powers of two times small integers) so that u = x A^T is a handful of terms and
    exactly representable in bf16; B is small integers scaled by a power of two.  Returns x, A, B, res, dy."""
    g = np.random.default_rng(seed)
    x = g.integers(-2, 3, size=(M, K)).astype(np.float64)
    x[:, min(5, K - 1)] += np.arange(M) % 7
    A = np.zeros((r, K))
    for j in range(r):
        cols = g.choice(K, size=min(4, K), replace=False)
        A[j, cols] = g.integers(-2, 3, size=len(cols))
    A[:, min(2, K - 1)] = (np.arange(r) % 3) - 1.0
    A *= 2.0 ** a_shift
    B = g.integers(-2, 3, size=(N, r)).astype(np.float64)
    B[:, min(1, r - 1)] += np.arange(N) % 3
    B *= 2.0 ** b_shift
    res = g.integers(-8, 9, size=(M, N)).astype(np.float64)
    dy = g.integers(-2, 3, size=(M, N)).astype(np.float64)
    dy[:, min(3, N - 1)] += np.arange(M) % 5
    return x, A, B, res, dy


def representable(v, dtype):
    """every value of v survives a round trip through the compute dtype"""
    t = torch.as_tensor(np.asarray(v, dtype=np.float64))
    return bool(torch.equal(t.to(TDT[dtype]).double(), t))
