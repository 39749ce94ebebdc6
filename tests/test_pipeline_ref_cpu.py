"""tests/pipeline_ref.smooth — the reference the GPU tests of fk_zscore_smooth_pad use — against scipy's gaussian_filter1d, including
trials shorter than the filter radius, where the reflection wraps more than once."""
import numpy as np
import pytest

from tests import pipeline_ref as PR


@pytest.mark.parametrize("sigma", [0.9, 1.0, 1.1])
@pytest.mark.parametrize("length", [1, 2, 3, 4, 5, 9, 64])
def test_smooth_is_scipys_reflect_filter(length, sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    z = np.random.default_rng(100 * length + int(10 * sigma)).standard_normal((length, 5))
    want = ndimage.gaussian_filter1d(z, sigma, axis=0, mode="reflect", radius=4)
    assert np.abs(PR.smooth(z, sigma) - want).max() < 1e-12


def test_block_stats_restatement():
    rng = np.random.default_rng(3)
    trials = [rng.standard_normal((n, 3)) for n in (4, 1, 6)]
    trials[0][:, 2] = trials[2][:, 2] = np.float32(0.3)               # the pipeline takes fp32 samples
    mean, std = PR.block_stats(trials, [0, 2, 0], 3)
    x = np.concatenate([trials[0], trials[2]])
    assert np.allclose(mean[0], x.mean(0)) and np.allclose(std[0, :2], x.std(0)[:2]) and std[0, 2] == 1.0
    assert np.array_equal(mean[1], np.zeros(3)) and np.array_equal(std[1], np.ones(3))          # no trials
    assert np.array_equal(mean[2], trials[1][0]) and np.array_equal(std[2], np.ones(3))         # one row: std 0 -> 1
