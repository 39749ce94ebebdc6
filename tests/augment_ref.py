"""The signal augmentation of csrc/augment.hip (fk_augment_patchify) restated in numpy / float64: every draw is a pure function of
(seed, step, sample, frame, channel), and this file is that function.  The rule is the comment of fk_augment_patchify in
include/franken_hip.h.  Integer decisions (drop, spans, shift) are made in uint64 / Python integer arithmetic; Philox is
tests/sample_ref.philox4x32_10, called on uint64 arrays (its expressions are the same on arrays as on Python ints).

    augment(x, cfg, words)                  -> y [B, T, C] float64, the exact values before the store's rounding
    augment(x, cfg, words, chain=np.float32) -> the same chain evaluated in numpy float32: its distance from the float64 values is the
                                               yardstick of the kernel's bound (tests/test_augment_gpu.py: 4 x its maximum on the case)
    forward(...)                            -> tok [B, (T / P) * C, ldp] in fk_patchify's layout, optionally rounded to 'fp32' / 'bf16'

`defect` plants one mistake (tests/test_augment_cpu.py shows that each breaks the GPU test's bound on a named case)."""
from dataclasses import dataclass

import numpy as np

from tests.day_adapter_ref import half_ulp, patchify, round_to  # noqa: F401  (the layout and the roundings are fk_patchify's)
from tests.sample_ref import philox4x32_10

TAG = 0xA0610000
WHITE, OFFSET, CHAN, SPAN, SHIFT = 1, 2, 3, 4, 5
MAX_SPANS = 8
DEFECTS = ("noise_by_source_frame", "offset_varies_in_time", "masks_before_noise", "noise_on_padding", "step_ignored", "shift_sign",
           "tail_reuses_lane0", "span_len_off_by_one")


@dataclass(frozen=True)
class Cfg:
    white_sd: float = 0.0
    offset_sd: float = 0.0
    chan_drop_p: float = 0.0
    time_shift: int = 0
    n_time_masks: int = 0
    time_mask_len: int = 0
    keep_padding: bool = True

    @property
    def noise(self):
        return self.white_sd > 0 or self.offset_sd > 0


def blocks(words, i0, i1, b, kind):
    """Philox blocks for broadcastable integer arrays (i0, i1, b): uint64 [..., 4], every entry below 2^32"""
    i0, i1, b = np.broadcast_arrays(np.asarray(i0, np.uint64), np.asarray(i1, np.uint64), np.asarray(b, np.uint64))
    key = (int(words[0]) & 0xFFFFFFFF, int(words[1]) & 0xFFFFFFFF)
    w = philox4x32_10(key, (i0, i1, b, np.full(i0.shape, TAG | kind, np.uint64)))
    return np.stack([np.asarray(v, np.uint64) for v in w], axis=-1)


def normals(w, chain=np.float64):
    """[..., 4] words -> [..., 4] standard normals: (w0, w1) -> normals 0, 1, (w2, w3) -> normals 2, 3, every step evaluated in `chain`"""
    f = chain
    out = np.empty(w.shape, f)
    for a in (0, 2):
        u1 = ((w[..., a] >> np.uint64(9)).astype(f) + f(0.5)) * f(2.0 ** -23)         # exact in fp32: 24 bits, never 0 or 1
        u2 = (w[..., a + 1] >> np.uint64(8)).astype(f) * f(2.0 ** -24)
        r = np.sqrt(f(-2.0) * np.log(u1))
        ang = f(2.0 * np.pi) * u2
        out[..., a], out[..., a + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


def white_normals(words, B, T, C, chain=np.float64, frames=None, tail_defect=False):
    """n_w [B, T, C]: block (t, c >> 2) of sample b, normal c & 3.  frames [B, T]: the frame number fed to the counter (default t)"""
    C4 = -(-C // 4)
    t = np.arange(T)[None, :, None] if frames is None else np.asarray(frames)[:, :, None]
    n = normals(blocks(words, t % (1 << 32), np.arange(C4)[None, None, :], np.arange(B)[:, None, None], WHITE), chain)   # [B, T, C4, 4]
    if tail_defect and C % 4:
        n[:, :, -1, :] = n[:, :, -1, :1]
    return n.reshape(B, T, C4 * 4)[:, :, :C]


def offset_normals(words, B, C, chain=np.float64, T=None):
    """n_o [B, C] (block (c >> 2, 0), normal c & 3); with T: the defect that feeds t as the second counter word, [B, T, C]"""
    C4 = -(-C // 4)
    if T is None:
        return normals(blocks(words, np.arange(C4)[None, :], 0, np.arange(B)[:, None], OFFSET), chain).reshape(B, C4 * 4)[:, :C]
    n = normals(blocks(words, np.arange(C4)[None, None, :], np.arange(T)[None, :, None], np.arange(B)[:, None, None], OFFSET), chain)
    return n.reshape(B, T, C4 * 4)[:, :, :C]


def drop_thresh(p):
    return min(int(np.floor(float(np.float32(p)) * 4294967296.0)), 0xFFFFFFFF)        # the knob travels as a C float


def dropped(words, B, C, p):
    """bool [B, C]: channel c of sample b is dropped iff w[c & 3] < thresh"""
    th = drop_thresh(p)
    if th == 0:
        return np.zeros((B, C), bool)
    C4 = -(-C // 4)
    w = blocks(words, np.arange(C4)[None, :], 0, np.arange(B)[:, None], CHAN).reshape(B, C4 * 4)[:, :C]
    return w < np.uint64(th)


def spans(words, B, T, n, Lmax, len_defect=False):
    """(start, len) int64 [B, n]"""
    if n == 0 or Lmax == 0:
        return np.zeros((B, 0), np.int64), np.zeros((B, 0), np.int64)
    w = blocks(words, np.arange(n)[None, :], 0, np.arange(B)[:, None], SPAN)
    ln = ((w[..., 0] >> np.uint64(8)) * np.uint64(Lmax if len_defect else Lmax + 1)) >> np.uint64(24)
    st = ((w[..., 1] >> np.uint64(8)) * (np.uint64(T + 1) - ln)) >> np.uint64(24)
    return st.astype(np.int64), ln.astype(np.int64)


def span_mask(words, B, T, n, Lmax, len_defect=False):
    """bool [B, T]: output frame t lies in a span"""
    st, ln = spans(words, B, T, n, Lmax, len_defect)
    t = np.arange(T)[None, :, None]
    return ((t >= st[:, None, :]) & (t < (st + ln)[:, None, :])).any(axis=2)


def shifts(words, B, S):
    """s_b int64 [B] in [-S, S]"""
    if S == 0:
        return np.zeros(B, np.int64)
    w = blocks(words, 0, 0, np.arange(B), SHIFT)
    return ((((w[..., 0] >> np.uint64(8)) * np.uint64(2 * S + 1)) >> np.uint64(24)).astype(np.int64)) - S


def augment(x, cfg, words, chain=np.float64, defect=None):
    """y [B, T, C] in `chain` (float64: the exact rule; float32: the same chain in fp32).  x is float32 data."""
    x = np.asarray(x, np.float32)
    B, T, C = x.shape
    f = chain
    if defect == "step_ignored":
        words = (words[0], 0)
    s = shifts(words, B, cfg.time_shift)
    if defect == "shift_sign":
        s = -s
    ts = np.arange(T)[None, :] - s[:, None]                                           # [B, T]
    inside = (ts >= 0) & (ts < T)
    src = np.where(inside[:, :, None], x[np.arange(B)[:, None], np.clip(ts, 0, T - 1)], np.float32(0)).astype(f)
    dead = ~inside
    if cfg.keep_padding and cfg.noise and defect != "noise_on_padding":
        dead = dead | ~(src != 0).any(axis=2)
    v = src
    if cfg.white_sd > 0:                                                              # a term whose sd is 0 is skipped
        nw = white_normals(words, B, T, C, f, frames=np.clip(ts, 0, T - 1) if defect == "noise_by_source_frame" else None,
                           tail_defect=defect == "tail_reuses_lane0")
        v = v + f(np.float32(cfg.white_sd)) * nw
    if cfg.offset_sd > 0:
        if defect == "offset_varies_in_time":
            v = v + f(np.float32(cfg.offset_sd)) * offset_normals(words, B, C, f, T=T)
        else:
            v = v + (f(np.float32(cfg.offset_sd)) * offset_normals(words, B, C, f))[:, None, :]
    masked = dropped(words, B, C, cfg.chan_drop_p)[:, None, :] | span_mask(words, B, T, cfg.n_time_masks, cfg.time_mask_len,
                                                                          defect == "span_len_off_by_one")[:, :, None]
    if defect == "masks_before_noise":                                                # the mask zeroes src, the noise lands on top
        v = np.where(masked, v - src, v)
        masked = np.zeros_like(masked)
    return np.where(dead[:, :, None] | masked, f(0), v)


def forward(x, cfg, words, P, ldp, dtype=None, chain=np.float64, defect=None):
    """tok [B, (T / P) * C, ldp] float64; dtype 'fp32' / 'bf16' applies the store's rounding, None leaves the exact values"""
    tok = patchify(augment(x, cfg, words, chain, defect).astype(np.float64), P, ldp)
    return tok if dtype is None else round_to(tok, dtype)


def bound(x, cfg, words, P, ldp):
    """(ref tok float64, scalar bound): 4 x the largest error of the numpy float32 chain against the float64 rule on this case; the
    device's own fp32 error is held to it (plus half a bf16 ulp for a bf16 store).  0 where no arithmetic happens: x passes bit for bit."""
    ref = forward(x, cfg, words, P, ldp)
    f32 = forward(x, cfg, words, P, ldp, chain=np.float32)
    return ref, 4.0 * float(np.max(np.abs(f32 - ref)))
