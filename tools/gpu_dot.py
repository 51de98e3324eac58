#!/usr/bin/env python3
"""Same-process A/B of the prepared dot product against `terms` launches of the prepared product.

  gpu_dot.py [--out FILE] [--resources FILE] [--repeats N]       driver: one child process per shape and term count, each under
                                                                 its own time limit; nothing runs after a step that failed
  gpu_dot.py --shape cfg2|cfg3 --terms T [--repeats N]           one point in this process; prints one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 output rows, cfg3 = n 1024 / 24-bit / 4,096 output rows; terms 2, 3, 4.  In one process,
after >= 0.15 s of warm launches, the four measurements
  dot_shared      tn_poly_dot_prepared_dev   bhat_sets = 1        one launch
  dot_per_set     tn_poly_dot_prepared_dev   bhat_sets = batch    one launch
  mult_shared     tn_poly_mult_prepared_dev  bhat_rows = 1        `terms` launches, one per term, each into a buffer of its own
  mult_per_row    tn_poly_mult_prepared_dev  bhat_rows = batch    `terms` launches
are timed interleaved `repeats` times, K rounds per sample between two events recorded on the stream the kernels run on.  The
mult_* baselines read the same buffers of a and bhat (batch * terms rows, taken as `terms` blocks of batch rows) and write
`terms` partial products; they leave out the additions a caller of the parent commit would need as well, so the comparison
is conservative.  Reported per measurement: median, min, max over the repeats and the spread (max - min) / median; the dot
product counts as faster only where its max is below the baseline's min (disjoint ranges).  --resources appends a file (the
resource table of the new kernels and the diff of the existing kernels' report against the parent commit, taken where the
library was built) to the report."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "cfg2": ("n=4096 60-bit", 4096, 1152921504606830593, 431606828070683274, 65536),
    "cfg3": ("n=1024 24-bit", 1024, 8380417, 5548360, 4096),
}
TERMS = (2, 3, 4)
STEP_TIMEOUT_S = 240
PAIRS = (("dot_shared", "mult_shared"), ("dot_per_set", "mult_per_row"))


def run_point(tag, terms, repeats):
    sys.path.insert(0, ROOT)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch = SHAPES[tag]
    plan = engine.Plan(n, q, psi)
    rows = batch * terms
    a = plan.fill_lcg(rows, 1, 2); b = plan.fill_lcg(rows, 2, 2)
    bhat = plan.prepare(b).tensor
    c = torch.empty((batch, n), dtype=a.dtype, device=a.device); c2 = torch.empty_like(c)
    parts = torch.empty((terms, batch, n), dtype=a.dtype, device=a.device)
    # (the C entry points directly: at cfg3 a launch is short enough for the Python wrappers' checks to show)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    pa, ph, pc, pc2, pp = (t.data_ptr() for t in (a, bhat, c, c2, parts))
    block = batch * n * plan.elem_bytes           # one term's block of batch rows in the baselines' view of a and bhat
    row = n * plan.elem_bytes

    def mult(shared):
        st_ = engine.TN_OK
        for j in range(terms):
            st_ |= lib.tn_poly_mult_prepared_dev(h, pa + j * block, ph + (j * row if shared else j * block), 1 if shared else batch, pp + j * block, batch, st)
        return st_

    launches = {
        "dot_shared": lambda: lib.tn_poly_dot_prepared_dev(h, pa, ph, 1, pc, batch, terms, st),
        "dot_per_set": lambda: lib.tn_poly_dot_prepared_dev(h, pa, ph, batch, pc2, batch, terms, st),
        "mult_shared": lambda: mult(True),
        "mult_per_row": lambda: mult(False),
    }
    # results first: the dot product is the sum of the products (first 64 output rows, both modes)
    for fn in launches.values():
        assert fn() == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()
    k = 64
    a3 = a[:k * terms].reshape(k, terms, n)
    identical = True
    for out, b3 in ((c, bhat[:terms].expand(k, terms, n)), (c2, bhat[:k * terms].reshape(k, terms, n))):
        acc = torch.zeros((k, n), dtype=a.dtype, device=a.device)
        for j in range(terms):
            p = plan.poly_mult_prepared(a3[:, j].contiguous(), engine.PreparedOperand(plan, b3[:, j].contiguous(), k))
            acc = acc + p
            acc = torch.where(acc >= q, acc - q, acc)
        identical = identical and bool(torch.equal(out[:k], acc))

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round (one dot launch, or `terms` product launches)

    est = sample(launches["mult_per_row"], 3)
    rounds = max(5, min(500, int(20.0 / est)))    # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for fn in launches.values():
            sample(fn, rounds)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds))
    out = {"shape": name, "batch": batch, "terms": terms, "rounds_per_sample": rounds, "repeats": repeats, "identical": identical,
           "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out["ms"][key] = {"median": med, "min": s[0], "max": s[-1], "spread": (s[-1] - s[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def report(results, resources):
    lines = ["Prepared dot product: one tn_poly_dot_prepared_dev launch against `terms` tn_poly_mult_prepared_dev launches (tools/gpu_dot.py)", ""]
    for r in results:
        lines.append(f"{r['shape']}, {r['batch']} output rows, terms {r['terms']}   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; first 64 rows identical to the summed products: {r['identical']}")
        for key in ("dot_shared", "mult_shared", "dot_per_set", "mult_per_row"):
            m = r["ms"][key]
            lines.append(f"  {key:12s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %")
        for dot, base in PAIRS:
            d, m = r["ms"][dot], r["ms"][base]
            verdict = "faster, ranges disjoint" if d["max"] < m["min"] else "NOT faster by disjoint ranges"
            lines.append(f"  {dot} / {base}: x{d['median'] / m['median']:6.3f}   {verdict}")
        lines.append("")
    if resources:
        with open(resources) as f:
            lines.append(f.read().rstrip())
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--terms", type=int, choices=TERMS)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_prepared_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.shape:
        return run_point(args.shape, args.terms or 2, args.repeats)
    results = []
    for tag in ("cfg2", "cfg3"):
        for terms in TERMS:
            step = f"{tag} terms {terms}"
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", tag, "--terms", str(terms), "--repeats", str(args.repeats)],
                                   stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                print(f"{step}: no result within {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
                return 124
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                print(f"{step}: exit status {r.returncode}; stopping", file=sys.stderr)
                return r.returncode if r.returncode > 0 else 1
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    text = report(results, args.resources)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
