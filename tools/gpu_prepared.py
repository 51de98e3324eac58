#!/usr/bin/env python3
"""Same-process A/B of the prepared-operand product against the three-transform product.

  gpu_prepared.py [--out FILE] [--resources FILE] [--repeats N]     driver: one child process per shape, each under its own
                                                                    time limit; nothing runs after a step that failed
  gpu_prepared.py --shape cfg2|cfg3 [--repeats N]                   one shape in this process; prints one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 rows, cfg3 = n 1024 / 24-bit / 4,096 rows (the benchmark's).  In one process, after
>= 0.15 s of warm launches, the four launches
  full      tn_poly_mult_dev            (a, b)       three transforms per row: the comparator
  per_row   tn_poly_mult_prepared_dev   bhat_rows = batch
  shared    tn_poly_mult_prepared_dev   bhat_rows = 1
  prepare   tn_prepare_dev              batch rows
are timed interleaved (full, per_row, shared, prepare, full, ...) `repeats` times, K launches per sample between two events
recorded on the stream the kernels run on.  Reported per launch: median, min, max over the repeats and the spread
(max - min) / median; ratios are medians against the median of `full`.  --resources appends a file (the diff of
`make -C tiny_ntt_amd/csrc resources` against the parent commit, taken where the library was built) to the report."""
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
STEP_TIMEOUT_S = 240


def run_shape(tag, repeats):
    sys.path.insert(0, ROOT)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch = SHAPES[tag]
    plan = engine.Plan(n, q, psi)
    a = plan.fill_lcg(batch, 1, 2); b = plan.fill_lcg(batch, 2, 2)
    c = torch.empty_like(a); c2 = torch.empty_like(a); bhat = torch.empty_like(a)
    per_row = plan.prepare(b, out=bhat)
    shared = plan.prepare(b[:1])
    # (the C entry points directly: at cfg3 a launch is short enough for the Python wrappers' checks to show)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    pa, pb, pc, pc2, ph, ps = (t.data_ptr() for t in (a, b, c, c2, bhat, shared.tensor))
    launches = {
        "full": lambda: lib.tn_poly_mult_dev(h, pa, pb, pc, batch, engine.VARIANT_FUSED, st),
        "per_row": lambda: lib.tn_poly_mult_prepared_dev(h, pa, ph, batch, pc2, batch, st),
        "shared": lambda: lib.tn_poly_mult_prepared_dev(h, pa, ps, 1, pc2, batch, st),
        "prepare": lambda: lib.tn_prepare_dev(h, pb, ph, batch, st),
    }
    # results first: the prepared product is the product
    assert launches["full"]() == engine.TN_OK and launches["per_row"]() == engine.TN_OK
    torch.cuda.synchronize()
    identical = bool(torch.equal(c, c2))
    assert launches["shared"]() == engine.TN_OK
    ref_shared = plan.poly_mult(a[:64], b[:1].expand(64, n).contiguous())
    torch.cuda.synchronize()
    identical = identical and bool(torch.equal(c2[:64], ref_shared))

    def sample(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k            # ms per launch

    est = sample(launches["full"], 3)
    k = max(5, min(500, int(20.0 / est)))         # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for fn in launches.values():
            sample(fn, k)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, k))
    out = {"shape": name, "batch": batch, "launches_per_sample": k, "repeats": repeats, "identical": identical, "build_id": engine.build_id(),
           "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out["ms"][key] = {"median": med, "min": s[0], "max": s[-1], "spread": (s[-1] - s[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def report(results, resources):
    lines = ["Prepared operand: tn_poly_mult_prepared_dev against tn_poly_mult_dev (tools/gpu_prepared.py)", ""]
    for r in results:
        lines.append(f"{r['shape']}, {r['batch']} rows   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['launches_per_sample']} launches each; results identical to the full product: {r['identical']}")
        full = r["ms"]["full"]["median"]
        for key in ("full", "per_row", "shared", "prepare"):
            m = r["ms"][key]
            lines.append(f"  {key:8s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %"
                         f"   x{m['median'] / full:6.3f} of full")
        lines.append("")
    if resources:
        lines.append("Register report (make -C tiny_ntt_amd/csrc resources) against the parent commit")
        lines.append("")
        with open(resources) as f:
            lines.append(f.read().rstrip())
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepared_operand_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.shape:
        return run_shape(args.shape, args.repeats)
    results = []
    for tag in ("cfg2", "cfg3"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", tag, "--repeats", str(args.repeats)],
                               stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{tag}: no result within {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{tag}: exit status {r.returncode}; stopping", file=sys.stderr)
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
