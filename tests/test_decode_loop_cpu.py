"""The arithmetic of GPT._run_steps, the one driver of every cached decode loop (models/gpt2_model.py): how many steps run, and when the
live count is read.  The step here is made of torch ops only, so the same cases run on the host (this file) and, eager and as a captured
graph, on the device (tests/test_eos_gpu.py)."""
import itertools

import pytest
import torch

from frankenstein_amd.models.gpt2_model import GPT

# max_new_tokens x check_every x die: the decode loop is dead (live = 0) once `die` steps have run, the caller's first step included
CASES = list(itertools.product((1, 2, 3, 4, 9), (1, 3, 8), (1, 2, 5, 100)))


def expected_steps(max_new_tokens, check_every, die):
    """the loop asks after every check_every-th step only: it stops at the smallest multiple of check_every >= die, or runs out"""
    return min(max_new_tokens, -(-die // check_every) * check_every)


def run_counted(device, max_new_tokens, check_every, die, use_graph=False, poll=True):
    """-> (steps _run_steps reports, calls of the step that ran).  The step counts itself and writes live = (1 + calls < die)."""
    count = torch.zeros(1, dtype=torch.int64, device=device)
    live = torch.full((1,), int(die > 1), dtype=torch.int32, device=device)

    def step():
        count.add_(1)
        live.copy_(count + 1 < die)

    if poll:
        n = GPT._run_steps(step, max_new_tokens, use_graph, live, check_every)
    else:
        n = GPT._run_steps(step, max_new_tokens, use_graph)
    return n, int(count.item())


@pytest.mark.parametrize("max_new_tokens,check_every,die", CASES)
def test_run_steps_stops_at_the_first_poll_behind_the_last_live_step(max_new_tokens, check_every, die):
    n, calls = run_counted("cpu", max_new_tokens, check_every, die)
    assert n == expected_steps(max_new_tokens, check_every, die) and calls == n - 1


@pytest.mark.parametrize("max_new_tokens", (1, 2, 3, 4, 9))
def test_run_steps_without_a_live_count_runs_every_step(max_new_tokens):
    assert run_counted("cpu", max_new_tokens, None, 1, poll=False) == (max_new_tokens, max_new_tokens - 1)
