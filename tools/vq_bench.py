"""Times the vector quantiser of the SoundStream tokenizer (profiles/vq_lookup.md): the fused lookup (fk_vq_assign, one launch) against
the chain it replaced (`VectorQuantize._lookup_chain`: norm, GEMM into an fp32 [R, K] similarity matrix, row argmax, gather, MSE), the
EMA codebook step before (`_ema_update_chain`, torch ops) and after (`_ema_update`: randint, gather, fk_vq_codebook_update), the
training-mode forward that holds both, and `init_codebook_` with 10 k-means rounds.

Shapes: K = 1024 codes, D = 64, R = 32 * 150 (cfg4) and R = 16 * 192 (the notebook size) rows, bf16 and fp32.  Every (R, dtype)
configuration runs in a fresh child process: device events around `iters` back-to-back calls, the variants alternated over `rounds`
rounds after a warm-up; the chain forward is listed twice, so the table shows the run-to-run spread of one and the same code next to
the difference between two.  Launch counts: the library's own launches in one call (its torch ops are listed in the profile).

    python tools/vq_bench.py [out.json]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [(32, 150, "bf16"), (32, 150, "fp32"), (16, 192, "bf16"), (16, 192, "fp32")]
KC, D = 1024, 64


def count_launches(f):
    """launches of the library's own kernels in one call of f (the fk_* entry points each enqueue one kernel; the torch ops of a
    variant are counted by reading its code: profiles/vq_lookup.md)"""
    from frankenstein_amd import kernels as K
    seen, orig = [], K.call
    K.call = lambda name, *a: (seen.append(name), orig(name, *a))[1]
    try:
        f()
    finally:
        K.call = orig
    return len(seen)


def child(B, T, dname, iters=200, rounds=7):
    import torch
    import frankenstein_amd as fa
    from frankenstein_amd import kernels as K
    from frankenstein_amd.models import vq_brain as vq
    fa.set_compute_dtype(dname)
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
    torch.manual_seed(0)
    m = vq.VectorQuantize(D, KC, kmeans_init=True).cuda()
    R = B * T
    x = (torch.randn(B, T, D, device="cuda") * (0.1 + 4.9 * torch.rand(B, T, 1, device="cuda"))).to(dt)
    x2 = x.reshape(R, D)
    assert K.vq_route(D, KC, dt)
    xn = torch.nn.functional.normalize(x2.float(), dim=-1)
    idx = K.vq_assign(x2, m._codebook.embed[0], False)[0]
    packed, counts, sums = K.vq_stats(KC, D, x.device)
    K.vq_assign(x2, m._codebook.embed[0], False, counts, sums)

    def mode(train):
        m.train(train)
        return m

    with torch.no_grad():
        variants = {
            "forward, chain": lambda: mode(False)._lookup_chain(x),
            "forward, fused": lambda: mode(False)(x),
            "forward, chain (again)": lambda: mode(False)._lookup_chain(x),
            "EMA step, torch chain": lambda: m._ema_update_chain(xn, idx),
            "EMA step, fused": lambda: m._ema_update(x2, packed),
            "training forward (lookup + EMA), chain": lambda: mode(True)._lookup_chain(x),
            "training forward (lookup + EMA), fused": lambda: mode(True)(x),
            "init_codebook_, 10 rounds": lambda: m.init_codebook_(x, iters=10),
        }
        launches = {name: count_launches(f) for name, f in variants.items()}
        for f in variants.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):
            for name, f in variants.items():
                n = iters // 10 if name.startswith("init") else iters
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(n):
                    f()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / n)
    res = {"R": R, "K": KC, "D": D, "dtype": dname, "iters": iters, "rounds": rounds, "us_per_call": {}}
    for name, ts in times.items():
        res["us_per_call"][name] = {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1),
                                    "launches": launches[name]}
    print("VQBENCH " + json.dumps(res), flush=True)


def main(out=None):
    results = []
    for B, T, dname in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(T), dname], capture_output=True, text=True,
                           timeout=300)
        line = next((l for l in r.stdout.splitlines() if l.startswith("VQBENCH ")), None)
        if r.returncode != 0 or line is None:
            raise RuntimeError(f"child {B}x{T} {dname} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        results.append(json.loads(line[len("VQBENCH "):]))
    for res in results:
        print(f"\nR = {res['R']}, K = {res['K']}, D = {res['D']}, {res['dtype']}")
        print("| variant | library launches | us per call, median (min - max) |\n|---|---|---|")
        for name, v in res["us_per_call"].items():
            print(f"| {name} | {v['launches']} | {v['median']} ({v['min']} - {v['max']}) |")
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
