"""Cases of the per-session input adapter tests (tests/test_day_adapter_cpu.py, tests/test_day_adapter_gpu.py): shapes, day patterns and
inputs on which a bookkeeping mistake is gross: delta is N(0, 1 / sqrt(C)) per day, non-symmetric and different for every day, bias is
different per day, so x @ delta[d] is as large as x itself.

SHAPES (B, T, C, P, ldp, n_days) are the issue's; ROUTE_SHAPES are added because the forward picks 32, 64 or 128 rows per workgroup from
B * ceil(T / rows) >= 256 and the small shapes all take 32: they are the smallest shapes that take 64 and 128 rows at one, two and four
column tiles per wave (C <= 128, <= 256, <= 512), with a ragged last tile and a C that is no multiple of 32."""
import numpy as np

SHAPES = [
    (3, 8, 8, 4, 4, 2),
    (4, 32, 16, 4, 32, 3),
    (2, 15, 40, 5, 32, 2),          # C no multiple of 16; padded columns
    (2, 200, 64, 25, 32, 4),
    (5, 50, 256, 25, 32, 24),       # days [23, 0, 23, 7, -1]
    (2, 33, 256, 1, 1, 2),          # fp32 only: the natural layout
    (1, 4, 512, 4, 4, 1),           # top of the envelope; one patch; B = 1
]
ROUTE_SHAPES = [
    (4, 4090, 8, 5, 8, 2),          # 64 rows per workgroup, one column tile
    (2, 16380, 8, 4, 4, 2),         # 128 rows, one column tile
    (8, 4090, 136, 5, 8, 2),        # 128 rows, two column tiles
    (4, 4090, 136, 5, 8, 2),        # 64 rows, two column tiles
    (8, 2045, 264, 5, 8, 2),        # 64 rows, four column tiles
]
PATTERNS = ("same", "different", "absent", "outrange", "null")


def fwd_rows(B, T, C):
    """rows per workgroup of fk_day_adapter_fwd (the rule of csrc/dayadapt.hip, restated)"""
    Cp = (C + 31) // 32 * 32
    G = 2 if C > 256 else 4
    while G > 1 and (32 * G * (Cp + 1) > 33 * 1024 or B * -(-T // (32 * G)) < 256):
        G //= 2
    return 32 * G


def days_of(pattern, B, n_days):
    if pattern == "null":
        return None
    if pattern == "same":
        return np.full(B, n_days - 1, dtype=np.int64)
    if pattern == "different":
        return (np.arange(B, dtype=np.int64) * 7 + 1) % n_days if n_days >= B else np.arange(B, dtype=np.int64) % n_days
    if pattern == "absent":                   # the last day never occurs (with one day: nobody has a valid day)
        return np.arange(B, dtype=np.int64) % (n_days - 1) if n_days > 1 else np.full(B, -1, dtype=np.int64)
    if pattern == "outrange":
        d = np.arange(B, dtype=np.int64) % n_days
        d[0] = n_days
        d[-1] = -1 if B > 1 else n_days
        return d
    if pattern == "mixed":
        return np.array([23, 0, 23, 7, -1], dtype=np.int64)
    raise KeyError(pattern)


class Case:
    def __init__(self, shape, pattern, seed):
        self.shape, self.pattern = shape, pattern
        self.B, self.T, self.C, self.P, self.ldp, self.n_days = shape
        self.seed = seed
        self.id = "B%d_T%d_C%d_P%d_ld%d_D%d-%s" % (*shape, pattern)

    @property
    def dtypes(self):
        return ("fp32",) if (self.P, self.ldp) == (1, 1) else ("fp32", "bf16")

    def inputs(self):
        """x, day, delta, bias, d_tok as numpy (fp32 values; day int64 or None); d_tok's padding columns hold garbage on purpose"""
        B, T, C, P, ldp, n_days = self.shape
        rng = np.random.default_rng(self.seed)
        x = rng.standard_normal((B, T, C)).astype(np.float32)
        delta = (rng.standard_normal((n_days, C, C)) / np.sqrt(C)).astype(np.float32)
        bias = (rng.standard_normal((n_days, C)) + np.arange(n_days)[:, None]).astype(np.float32)
        d_tok = rng.standard_normal((B, (T // P) * C, ldp)).astype(np.float32)
        return x, days_of(self.pattern, B, n_days), delta, bias, d_tok


def _cases(shapes, patterns_of):
    out = []
    for i, s in enumerate(shapes):
        for j, p in enumerate(patterns_of(s)):
            out.append(Case(s, p, 1000 + 17 * i + j))
    return out


CASES = _cases(SHAPES, lambda s: PATTERNS + (("mixed",) if s[0] == 5 and s[5] == 24 else ()))
ROUTE_CASES = _cases(ROUTE_SHAPES, lambda s: ("different", "outrange"))
BY_ID = {c.id: c for c in CASES + ROUTE_CASES}
