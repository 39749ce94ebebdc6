"""Cases of the signal-augmentation tests (tests/test_augment_cpu.py, tests/test_augment_gpu.py): the shapes (B, T, C, P, ldp) and, for
each, the variants: every knob alone, all together, zero padding (a padded tail per sample and one interior all-zero frame), a shift that
moves padding into range, a span as long as the trial, 8 overlapping spans, a drop probability near 0 and near 1, and a second step word.
The knobs scale with T so that every variant is legal at T = 8 (time_shift < T, time_mask_len <= T)."""
import numpy as np

from tests.augment_ref import Cfg

SHAPES = [
    (2, 8, 8, 4, 4),                # smallest shape
    (3, 15, 40, 5, 32),             # padded columns, P * C4 no multiple of the block
    (2, 12, 6, 3, 4),               # C % 4 != 0: the last Philox block of a row is partial
    (2, 50, 256, 25, 32),           # one real patch geometry
    (4, 32, 16, 1, 1),              # fp32 only: signal mode
]
STEP = 3


def variants(T):
    q = max(1, T // 4)
    return {
        "white": (Cfg(white_sd=0.5), False, STEP),
        "offset": (Cfg(offset_sd=0.3), False, STEP),
        "chan_drop": (Cfg(chan_drop_p=0.3), False, STEP),
        "time_shift": (Cfg(time_shift=q), False, STEP),
        "time_masks": (Cfg(n_time_masks=2, time_mask_len=T // 2), False, STEP),
        "all": (Cfg(0.5, 0.3, 0.2, q, 3, T // 3), True, STEP),
        "all_step2": (Cfg(0.5, 0.3, 0.2, q, 3, T // 3), True, STEP + 1),
        "padded": (Cfg(white_sd=0.5, offset_sd=0.3), True, STEP),
        "padded_nokeep": (Cfg(white_sd=0.5, keep_padding=False), True, STEP),
        "shift_pad": (Cfg(white_sd=0.5, time_shift=q + 1), True, STEP),
        "mask_full": (Cfg(white_sd=0.5, n_time_masks=1, time_mask_len=T), False, STEP),
        "spans8": (Cfg(offset_sd=0.3, n_time_masks=8, time_mask_len=T // 2), False, STEP),
        "drop_lo": (Cfg(white_sd=0.5, chan_drop_p=0.02), False, STEP),
        "drop_hi": (Cfg(white_sd=0.5, chan_drop_p=0.98), False, STEP),
    }


class Case:
    def __init__(self, shape, name, cfg, padded, step, seed):
        self.shape, self.name, self.cfg, self.padded = shape, name, cfg, padded
        self.B, self.T, self.C, self.P, self.ldp = shape
        self.seed = seed
        self.words = ((0x2545F491 * (seed + 1)) & 0x7FFFFFFF, step)
        self.id = "B%d_T%d_C%d_P%d_ld%d-%s" % (*shape, name)

    @property
    def dtypes(self):
        return ("fp32",) if (self.P, self.ldp) == (1, 1) else ("fp32", "bf16")

    def x(self):
        """fp32 [B, T, C] z-scored-like data; padded: sample b's last (T // 4) + b frames are zero (at least one), and frame 1 of sample 0"""
        B, T, C = self.B, self.T, self.C
        x = np.random.default_rng(self.seed).standard_normal((B, T, C)).astype(np.float32)
        if self.padded:
            for b in range(B):
                x[b, T - max(1, T // 4) - b:] = 0.0
            x[0, 1] = 0.0
        return x


def _cases():
    out = []
    for i, s in enumerate(SHAPES):
        for j, (name, (cfg, padded, step)) in enumerate(variants(s[1]).items()):
            out.append(Case(s, name, cfg, padded, step, 2000 + 31 * i + (j if name != "all_step2" else j - 1)))   # all_step2: all's data and seed
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
