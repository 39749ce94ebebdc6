"""The vector-quantiser kernels (csrc/vq.hip) and their users (engine.VQLookupFn, models/vq_brain.py) against the float64 restatement in
tests/vq_ref.py.  The inputs are fixed (vq_ref.lookup_inputs / planted); tests/test_vq_cpu.py checks on the CPU that the reference's own
top-2 similarity gap leaves (almost) no row of them inside the near-tie band the index comparison skips."""
import functools

import numpy as np
import pytest
import torch

from tests import vq_ref as VR

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STRIDED = {(65, 64, 16), (300, 1031, 64)}          # cases run with a row stride of D + 8 elements


@pytest.fixture(autouse=True)
def _keep_compute_dtype():
    import frankenstein_amd as fa
    from frankenstein_amd import engine as E
    before = E.compute_dtype()
    yield
    fa.set_compute_dtype(before)


def _bf16_ulp(v):
    """spacing of bf16 (8 significant bits) at |v|"""
    v = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(v)) - 7)


def _round(t, dtype):
    return t.to(dtype).to(torch.float64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(R, Kc, D, dname):
    """inputs as the kernel sees them and the float64 lookup from the same values, computed once per case"""
    x32, codes = VR.lookup_inputs(R, Kc, D)
    xt = torch.from_numpy(x32).to(DTYPES[dname])
    xv = xt.to(torch.float64).numpy()
    idx, gap, xn, _ = VR.lookup(xv, codes)
    return xt, torch.from_numpy(codes), xv, codes.astype(np.float64), idx, gap, xn


def _device_rows(xt, ld):
    R, D = xt.shape
    if ld == D:
        return xt.cuda().contiguous()
    base = torch.full((R, ld), float("nan"), dtype=xt.dtype, device="cuda")       # the padding is never read: NaN would poison everything
    base[:, :D] = xt.cuda()
    return base[:, :D]


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("case", VR.LOOKUP_CASES)
def test_lookup_matches_float64(case, dname):
    from frankenstein_amd import kernels as K
    R, Kc, D = case
    xt, codes_t, xv, codes, ref_idx, gap, xn = _case(R, Kc, D, dname)
    x = _device_rows(xt, D + 8 if case in STRIDED else D)
    codes_d = codes_t.cuda()
    packed, counts, sums = K.vq_stats(Kc, D, "cuda")
    idx, q, commit = K.vq_assign(x, codes_d, True, counts, sums, commit_scale=1.0)
    torch.cuda.synchronize()
    idx_h = idx.cpu().numpy()
    sure = gap >= VR.GAP
    print(f"{case} {dname}: excluded {int((~sure).sum())} of {R}, disagreeing {(idx_h != ref_idx).sum()}, smallest gap {gap.min():.3g}")
    assert (~sure).mean() <= 0.01
    assert idx_h.min() >= 0 and idx_h.max() < Kc
    np.testing.assert_array_equal(idx_h[sure], ref_idx[sure])
    # everything below is a function of the assignment: the reference takes the kernel's index on the (at most 1 %) excluded rows
    use = np.where(sure, ref_idx, idx_h)
    q_ref = codes_t[torch.from_numpy(use)].to(DTYPES[dname])
    assert torch.equal(q.cpu(), q_ref), "q is not bit-equal to round(codes[idx])"
    want = VR.commit_sum(xv, q_ref.to(torch.float64).numpy())
    got = float(commit.cpu()[0])
    print(f"  commit {got:.8g} vs {want:.8g} (rel {abs(got - want) / want:.3g})")
    assert abs(got - want) <= 1e-4 * want
    c_ref, s_ref = VR.stats(xn, use, Kc)
    np.testing.assert_array_equal(counts.cpu().numpy(), c_ref)
    mean_err = np.abs(sums.cpu().numpy().astype(np.float64) - s_ref).max(axis=1) / np.maximum(c_ref, 1)
    print(f"  sums / count: max error {mean_err.max():.3g}")
    assert mean_err.max() <= 1e-4


def test_lookup_without_optional_outputs_returns_the_same_indices():
    """idx alone (no q, no statistics, no commitment sum): the early-exit form of the launch used by nothing but callers that want ids"""
    from frankenstein_amd import kernels as K
    xt, codes_t, *_ = _case(257, 1000, 64, "fp32")
    full = K.vq_assign(xt.cuda(), codes_t.cuda(), True, None, None, 1.0)
    idx, q, commit = K.vq_assign(xt.cuda(), codes_t.cuda(), False)
    assert q is None and commit is None and torch.equal(idx, full[0])


@pytest.mark.parametrize("dname", sorted(DTYPES))
def test_exact_ties_return_the_lower_index(dname):
    """code j repeated at j' > j: inside one chunk of 32, across a chunk boundary, in a later chunk of the same wave (8 chunks on), in a
    chunk of another wave, and in the tail chunk of K = 1031 (codes 1024..1030)"""
    from frankenstein_amd import kernels as K
    _, codes_t, *_ = _case(300, 1031, 64, "fp32")
    codes = codes_t.clone()
    pairs = [(10, 20), (31, 32), (3, 3 + 256), (5, 40), (700, 1029), (1025, 1030), (0, 1023)]
    for j, jj in pairs:
        codes[jj] = codes[j]
    rows = torch.cat([3.0 * codes[[j for j, _ in pairs]], 0.25 * codes[[jj for _, jj in pairs]]]).to(DTYPES[dname])
    idx, _, _ = K.vq_assign(rows.cuda(), codes.cuda(), False)
    assert idx.cpu().tolist() == [j for j, _ in pairs] * 2


@pytest.mark.parametrize("dname", sorted(DTYPES))
def test_every_code_index_is_reachable(dname):
    """x_i = 3 e_pi(i) for a permutation pi of all K = 1031 codes returns exactly pi: a misplaced or masked code shows as a wrong id"""
    from frankenstein_amd import kernels as K
    _, codes_t, *_ = _case(300, 1031, 64, "fp32")
    perm = torch.from_numpy(np.random.default_rng(5).permutation(1031))
    rows = (3.0 * codes_t[perm]).to(DTYPES[dname])
    idx, q, _ = K.vq_assign(rows.cuda(), codes_t.cuda(), True)
    assert torch.equal(idx.cpu(), perm)
    assert torch.equal(q.cpu(), codes_t[perm].to(DTYPES[dname]))


def test_forward_is_deterministic_and_graph_replay_has_the_same_bits():
    from frankenstein_amd import kernels as K
    xt, codes_t, *_ = _case(513, 1024, 64, "bf16")
    x, codes = xt.cuda(), codes_t.cuda()
    a = K.vq_assign(x, codes, True, None, None, 0.25 / x.numel())
    b = K.vq_assign(x, codes, True, None, None, 0.25 / x.numel())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        K.vq_assign(x, codes, True, None, None, 0.25 / x.numel())
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        c = K.vq_assign(x, codes, True, None, None, 0.25 / x.numel())
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("R,D", [(65, 16), (257, 64)])
def test_backward_matches_float64(R, D, dname):
    """dx = dq + dcommit * 2 * commitment_weight / (R D) * (x - q) through autograd (engine.VQLookupFn): loss = sum(w * q) + 3 * commit"""
    from frankenstein_amd import engine as E
    dt, cw = DTYPES[dname], 0.25
    rng = np.random.default_rng(R + D)
    x = torch.from_numpy(rng.standard_normal((1, R, D)).astype(np.float32) * 2).to(dt).cuda().requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((1, R, D)).astype(np.float32)).to(dt).cuda()
    codes = torch.from_numpy(VR.normalize(rng.standard_normal((40, D))).astype(np.float32)).cuda()
    q, idx, commit = E.VQLookupFn.apply(x, codes, cw)
    assert not idx.requires_grad and commit.dtype == torch.float32 and commit.dim() == 0
    ((q.float() * w.float()).sum() + 3.0 * commit).backward()
    ref = VR.backward(_round(x.detach(), dt), _round(q.detach(), dt), _round(w, dt), 3.0, cw)
    err = np.abs(x.grad.to(torch.float64).cpu().numpy() - ref)
    if dname == "fp32":
        print(f"dx fp32: max error {err.max():.3g}")
        assert err.max() <= 1e-6
    else:
        print(f"dx bf16: max error in ulps {(err / _bf16_ulp(ref)).max():.3g}")
        assert (err <= _bf16_ulp(ref)).all()
    # the commitment term alone (no gradient arrives through q) and the straight-through term alone
    x2 = x.detach().clone().requires_grad_(True)
    E.VQLookupFn.apply(x2, codes, cw)[2].backward()
    ref_c = VR.backward(_round(x2.detach(), dt), _round(q.detach(), dt), np.zeros((1, R, D)), 1.0, cw)
    err_c = np.abs(x2.grad.to(torch.float64).cpu().numpy() - ref_c)
    assert (err_c <= (1e-6 if dname == "fp32" else _bf16_ulp(ref_c))).all()
    x3 = x.detach().clone().requires_grad_(True)
    (E.VQLookupFn.apply(x3, codes, cw)[0].float() * w.float()).sum().backward()
    assert torch.equal(x3.grad, w)


def _ema_state(Kc, D, R, seed):
    """buffers, and the counts / sums of a real lookup of R rows, as float64 arrays"""
    rng = np.random.default_rng(seed)
    emb = VR.normalize(rng.standard_normal((Kc, D)))
    cs = rng.uniform(3.0, 12.0, Kc)
    avg = emb * cs[:, None] * rng.uniform(0.8, 1.2, (Kc, 1))
    x = (rng.standard_normal((R, D)) * rng.uniform(0.1, 5.0, (R, 1))).astype(np.float32).astype(np.float64)
    idx, _, xn, _ = VR.lookup(x, emb)
    counts, sums = VR.stats(xn, idx, Kc)
    return emb, avg, cs, counts, sums, x


def _close(got, ref, bound=1e-5):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got.to(torch.float64).cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("Kc,D,packed", [(33, 16, False), (1031, 64, True)])
def test_ema_update_matches_float64(Kc, D, packed):
    from frankenstein_amd import kernels as K
    emb, avg, cs, counts, sums, _ = _ema_state(Kc, D, 300, 11 + Kc)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().contiguous()
    embed, embed_avg, cluster = f(emb), f(avg), f(cs)
    if packed:                                   # the product's layout: sums | counts in one [K, D + 1] tensor
        pk = torch.cat([f(sums), f(counts)[:, None]], dim=1).contiguous()
        c_d, s_d = pk[:, D], pk[:, :D]
    else:
        c_d, s_d = f(counts), f(sums)
    seed = torch.full((Kc, D), float("nan"), device="cuda")          # dead = 0: no code is re-seeded, the seed is never used
    before = (_round(embed, torch.float32), _round(embed_avg, torch.float32), _round(cluster, torch.float32))
    K.vq_codebook_update(embed, c_d, s_d, K.VQ_EMA, embed_avg, cluster, seed, 0.8, 1e-5, 0.0)
    e1, a1, c1, dead = VR.ema(*before, _round(c_d, torch.float32), _round(s_d, torch.float32), 0.8, 1e-5, 0.0)
    errs = (_close(cluster, c1), _close(embed_avg, a1), _close(embed, e1))
    print(f"EMA K={Kc} D={D}: errors relative to max(1, |ref|): cluster_size {errs[0]:.3g}, embed_avg {errs[1]:.3g}, embed {errs[2]:.3g}")
    assert not dead.any() and max(errs) <= 1e-5


def test_dead_codes_are_reseeded_from_the_batch():
    from frankenstein_amd import kernels as K
    Kc, D, R, dead_thr = 70, 16, 300, 2.0
    emb, avg, cs, counts, sums, x = _ema_state(Kc, D, R, 23)
    chosen = np.array([0, 31, 32, 63, 64, 69])
    cs[chosen], counts[chosen], sums[chosen] = 0.1, 0.0, 0.0         # 0.8 * 0.1 < 2: below the threshold; every other code stays above
    pick = np.random.default_rng(2).integers(0, R, Kc)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().contiguous()
    embed, embed_avg, cluster, seed = f(emb), f(avg), f(cs), f(x[pick])
    before = (_round(embed, torch.float32), _round(embed_avg, torch.float32), _round(cluster, torch.float32))
    K.vq_codebook_update(embed, f(counts), f(sums), K.VQ_EMA, embed_avg, cluster, seed, 0.8, 1e-5, dead_thr)
    e1, a1, c1, dead = VR.ema(*before, counts, sums, 0.8, 1e-5, dead_thr, seed=x[pick])
    assert sorted(np.flatnonzero(dead)) == sorted(chosen)
    got = embed.to(torch.float64).cpu().numpy()
    xn = VR.normalize(x)
    cos = (got[chosen] @ xn.T).max(axis=1)
    print(f"re-seeded codes: |e| - 1 up to {np.abs(np.linalg.norm(got[chosen], axis=1) - 1).max():.3g}, best cosine with the batch >= {cos.min():.8f}")
    assert np.abs(np.linalg.norm(got[chosen], axis=1) - 1).max() <= 1e-6 and cos.min() >= 1 - 1e-5
    assert torch.equal(embed_avg[chosen], embed[chosen] * dead_thr) and (cluster[chosen] == dead_thr).all()
    assert max(_close(cluster, c1), _close(embed_avg, a1), _close(embed, e1)) <= 1e-5       # every other code: the float64 EMA


def _vq(Kc, D):
    from frankenstein_amd.models import vq_brain as vq
    return vq.VectorQuantize(D, Kc, kmeans_init=True).cuda()


def test_kmeans_init_matches_the_float64_lloyd_iteration():
    import frankenstein_amd as fa
    from frankenstein_amd import kernels as K
    fa.set_compute_dtype("fp32")
    x, init, _ = VR.planted()
    R, (Kc, D) = x.shape[0], init.shape
    xn, means = VR.normalize(x), init.astype(np.float64)
    for _ in range(3):
        prev = means
        means, idx, counts, gap, _ = VR.kmeans_round(xn, means)
        assert gap >= 1e-4
    m = _vq(Kc, D)
    m._codebook.initted.fill_(False)
    m.init_codebook_(torch.from_numpy(x).cuda().view(4, R // 4, D), iters=3, init_means=torch.from_numpy(init))
    cb = m._codebook
    err = np.abs(cb.embed[0].to(torch.float64).cpu().numpy() - means).max()
    print(f"k-means, 3 rounds: embed error {err:.3g}")
    assert err <= 1e-5
    np.testing.assert_array_equal(cb.cluster_size[0].cpu().numpy(), counts)          # the last round's assignment, counted
    assert float(cb.cluster_size.sum()) == R and bool(cb.initted)
    assert torch.equal(cb.embed_avg[0], cb.embed[0] * cb.cluster_size[0][:, None])
    final_idx, _, _ = K.vq_assign(torch.from_numpy(x).cuda(), cb.embed[0], False)
    np.testing.assert_array_equal(final_idx.cpu().numpy(), VR.lookup(x.astype(np.float64), means)[0])
    assert np.abs(np.linalg.norm(cb.embed[0].cpu().numpy().astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_kmeans_random_start_never_gets_worse():
    """mean best similarity over the rows, evaluated in float64 from the codebook after every round (rounds run one at a time, each
    starting from the last one's means).  Lloyd's iteration is monotone; 1e-6 covers the fp32 rounding of the stored means."""
    import frankenstein_amd as fa
    fa.set_compute_dtype("fp32")
    x, init, _ = VR.planted()
    Kc, D = init.shape
    xn = VR.normalize(x)
    score = lambda m: float((xn @ m._codebook.embed[0].to(torch.float64).cpu().numpy().T).max(axis=1).mean())
    torch.manual_seed(3)
    m = _vq(Kc, D)
    xd = torch.from_numpy(x).cuda()
    m.init_codebook_(xd, iters=0)                       # the random start alone: K distinct rows of x, normalised
    start = m._codebook.embed[0].to(torch.float64).cpu().numpy()
    assert np.abs(start @ xn.T).max(axis=1).min() >= 1 - 1e-6
    scores = [score(m)]
    for _ in range(4):
        m.init_codebook_(xd, iters=1, init_means=m._codebook.embed[0])
        scores.append(score(m))
    print("mean best similarity per round:", " ".join(f"{s:.6f}" for s in scores))
    assert all(b >= a - 1e-6 for a, b in zip(scores, scores[1:])) and scores[-1] > scores[0]


def test_kmeans_empty_cluster_keeps_its_mean():
    import frankenstein_amd as fa
    fa.set_compute_dtype("fp32")
    x, init, j = VR.planted_with_empty_cluster()                                # mean 5 points away from every row: nothing selects it
    assert j == 5
    Kc, D = init.shape
    m = _vq(Kc, D)
    m.init_codebook_(torch.from_numpy(x).cuda(), iters=2, init_means=torch.from_numpy(init))
    cb = m._codebook
    assert torch.equal(cb.embed[0][5].cpu(), torch.from_numpy(init[5]))
    assert float(cb.cluster_size[0][5]) == 0 and float(cb.embed_avg[0][5].abs().sum()) == 0
    assert float(cb.cluster_size.sum()) == x.shape[0]


def _soundstream(D=16):
    from frankenstein_amd import synth
    from frankenstein_amd.models import vq_brain as vq
    torch.manual_seed(0)
    net = vq.SoundStream(C=32, D=D, codebook_size=64, n_electrodes=16).cuda()
    return net, torch.from_numpy(synth.make_inputs(4, 64, 16)).cuda()


def test_model_fused_forward_matches_the_chain_fp32():
    import frankenstein_amd as fa
    from frankenstein_amd.models.brainformer import _prep
    fa.set_compute_dtype("fp32")
    net, x = _soundstream()
    net.eval()
    with torch.no_grad():
        e = _prep(net.encoder(x))
        q1, i1, c1 = net.quantizer(e)
        q0, i0, c0 = net.quantizer._lookup_chain(e)
    assert q1.shape == q0.shape and i1.shape == i0.shape == (4, 16) and q1.dtype == q0.dtype and i1.dtype == torch.int64 and c1.shape == c0.shape
    _, gap, _, _ = VR.lookup(e.reshape(-1, 16).to(torch.float64).cpu().numpy(), net.quantizer._codebook.embed[0].to(torch.float64).cpu().numpy())
    sure = torch.from_numpy(gap >= VR.GAP).cuda().view(4, 16)
    assert (~sure).float().mean() <= 0.01
    assert torch.equal(i1[sure], i0[sure]) and torch.equal(q1[sure], q0[sure])
    print(f"commit loss fused {float(c1):.9g} chain {float(c0):.9g}")
    assert abs(float(c1) - float(c0)) <= 1e-6            # 64 rows: the 1 % above leaves no row out, the two paths chose the same codes
    loss1, _ = net(x)
    assert net.quantizer.last_counts is None and torch.isfinite(loss1)


def test_model_training_with_kmeans_init():
    import frankenstein_amd as fa
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("fp32")
    net, x = _soundstream()
    net.train()
    before = net.quantizer._codebook.embed.clone()
    net.init_codebook(x)
    cb = net.quantizer._codebook
    assert not torch.equal(before, cb.embed) and float(cb.cluster_size.sum()) == 64 and bool(cb.initted)
    # the lookup's own counts give the perplexity calculate_perp() computes from the indices
    with torch.no_grad():
        e = net.encoder(x)
        _, idx, _ = net.quantizer(e)
        assert torch.equal(net._perp_of_counts(net.quantizer.last_counts), net.calculate_perp(idx))
    opt = tu.FusedAdamW(net, lr=2e-3, weight_decay=0.0)
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=2e-3)
    losses = [float(tu.train_step(net, (x, None, None), opt, step, cfg)) for step in range(3)]
    assert all(np.isfinite(losses)), losses
    assert torch.isfinite(net.last_perplexity) and 1.0 <= float(net.last_perplexity) <= 64.0
    assert torch.isfinite(cb.embed).all() and torch.allclose(cb.embed[0].norm(dim=-1), torch.ones(64, device="cuda"), atol=1e-5)
    assert net.encoder.layers[0].weight.abs().sum() > 0


def test_out_of_envelope_takes_the_chain():
    """D = 132 (fp32) is outside fk_vq_route's envelope and runs through `_lookup_chain` as before; D = 6 is routed there too (the chain's
    own GEMM needs D % 4 == 0 in fp32, as it always did, so that call is only observed, not run)."""
    import frankenstein_amd as fa
    from frankenstein_amd import kernels as K
    from frankenstein_amd.models import vq_brain as vq
    fa.set_compute_dtype("fp32")
    assert not K.vq_route(132, 64, torch.float32) and not K.vq_route(6, 64, torch.float32)
    torch.manual_seed(1)
    m = vq.VectorQuantize(132, 64).cuda().train()
    x = torch.randn(2, 40, 132, device="cuda", requires_grad=True)
    q, idx, commit = m(x)
    (q.sum() + commit).backward()
    assert q.shape == (2, 40, 132) and idx.shape == (2, 40) and torch.isfinite(commit) and torch.isfinite(x.grad).all()
    ref = (torch.nn.functional.normalize(x.detach().reshape(-1, 132), dim=-1) @ q.detach().reshape(-1, 132).t()).diagonal()
    assert m.last_counts is None and float(ref.min()) > 0
    seen = []
    m6 = vq.VectorQuantize(6, 64).cuda().eval()
    m6._lookup_chain = lambda t: seen.append(tuple(t.shape)) or "chain"
    assert m6(torch.randn(2, 8, 6, device="cuda")) == "chain" and seen == [(2, 8, 6)]
