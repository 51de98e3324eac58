#!/usr/bin/env python3
"""Same-process A/B of the gadget dot product against decompose-then-dot on the same buffers.

  gpu_gadget.py [--out FILE] [--resources FILE] [--repeats N] [--unsigned]   driver: one child process per shape and term count, each
                                                                             under its own time limit; nothing runs after a step that failed
  gpu_gadget.py --shape cfg2|cfg3 --terms T [--repeats N] [--unsigned]       one point in this process; prints one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 output rows (base_log 30, 20, 15 for terms 2, 3, 4), cfg3 = n 1024 / 24-bit / 4,096 output
rows (base_log 12, 8, 6).  Balanced digits unless --unsigned.  In one process, after >= 0.15 s of warm launches, the six measurements
  gadget_shared   tn_poly_gadget_dot_prepared_dev   bhat_sets = 1       one launch
  gadget_per_set  tn_poly_gadget_dot_prepared_dev   bhat_sets = batch   one launch
  base_shared     tn_gadget_decompose_dev, then tn_poly_dot_prepared_dev on its output (bhat_sets = 1): two launches
  base_per_set    the same with bhat_sets = batch
  dot_shared      tn_poly_dot_prepared_dev alone on digits decomposed beforehand (bhat_sets = 1): the floor of the old path,
  dot_per_set     reported, not a gate
are timed interleaved `repeats` times, K rounds per sample between two events recorded on the stream the kernels run on.  The
baseline is what a caller has without the fused call, with this library's own decompose kernel in place of one of theirs.
Reported per measurement: median, min, max over the repeats and the spread (max - min) / median; the fused call counts as faster
only where its max is below the baseline's min (disjoint ranges).  --resources appends a file (the resource table of the new
kernels and the comparison of the existing kernels' report with the parent commit, taken where the library was built)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "cfg2": ("n=4096 60-bit", 4096, 1152921504606830593, 431606828070683274, 65536, {2: 30, 3: 20, 4: 15}),
    "cfg3": ("n=1024 24-bit", 1024, 8380417, 5548360, 4096, {2: 12, 3: 8, 4: 6}),
}
TERMS = (2, 3, 4)
STEP_TIMEOUT_S = 240
PAIRS = (("gadget_shared", "base_shared", "dot_shared"), ("gadget_per_set", "base_per_set", "dot_per_set"))


def run_point(tag, terms, repeats, balanced):
    sys.path.insert(0, ROOT)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED if balanced else 0
    plan = engine.Plan(n, q, psi)
    a = plan.fill_lcg(batch, 1, 2); b = plan.fill_lcg(batch * terms, 2, 2)
    bhat = plan.prepare(b).tensor
    c = torch.empty((batch, n), dtype=a.dtype, device=a.device); c2 = torch.empty_like(c)
    cb = torch.empty_like(c); cb2 = torch.empty_like(c)
    digits = torch.empty((batch, terms, n), dtype=a.dtype, device=a.device)
    fixed = plan.gadget_decompose(a, terms, w, balanced)            # the floor's input: decomposed once, outside the timing
    # (the C entry points directly: at cfg3 a launch is short enough for the Python wrappers' checks to show)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    pa, ph, pc, pc2, pcb, pcb2, pd, pf = (t.data_ptr() for t in (a, bhat, c, c2, cb, cb2, digits, fixed))

    def base(sets, out):
        return lib.tn_gadget_decompose_dev(h, pa, pd, batch, terms, w, flags, st) | lib.tn_poly_dot_prepared_dev(h, pd, ph, sets, out, batch, terms, st)

    launches = {
        "gadget_shared": lambda: lib.tn_poly_gadget_dot_prepared_dev(h, pa, ph, 1, pc, batch, terms, w, flags, st),
        "gadget_per_set": lambda: lib.tn_poly_gadget_dot_prepared_dev(h, pa, ph, batch, pc2, batch, terms, w, flags, st),
        "base_shared": lambda: base(1, pcb),
        "base_per_set": lambda: base(batch, pcb2),
        "dot_shared": lambda: lib.tn_poly_dot_prepared_dev(h, pf, ph, 1, pcb, batch, terms, st),
        "dot_per_set": lambda: lib.tn_poly_dot_prepared_dev(h, pf, ph, batch, pcb2, batch, terms, st),
    }
    # results first: the fused call is bit-identical to the two launches (every row, both sharings)
    for fn in launches.values():
        assert fn() == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()
    identical = bool(torch.equal(c, cb)) and bool(torch.equal(c2, cb2)) and bool(torch.equal(digits, fixed))

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round (one fused launch, or decompose + dot)

    est = sample(launches["base_per_set"], 3)
    rounds = max(5, min(500, int(20.0 / est)))    # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for fn in launches.values():
            sample(fn, rounds)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds))
    out = {"shape": name, "batch": batch, "terms": terms, "base_log": w, "balanced": balanced, "rounds_per_sample": rounds, "repeats": repeats,
           "identical": identical, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out["ms"][key] = {"median": med, "min": s[0], "max": s[-1], "spread": (s[-1] - s[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def report(results, resources):
    lines = ["Gadget dot product: one tn_poly_gadget_dot_prepared_dev launch against tn_gadget_decompose_dev + tn_poly_dot_prepared_dev (tools/gpu_gadget.py)", ""]
    for r in results:
        lines.append(f"{r['shape']}, {r['batch']} output rows, terms {r['terms']}, base_log {r['base_log']}, {'balanced' if r['balanced'] else 'unsigned'} digits"
                     f"   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every row identical to decompose + dot: {r['identical']}")
        for key in ("gadget_shared", "base_shared", "dot_shared", "gadget_per_set", "base_per_set", "dot_per_set"):
            m = r["ms"][key]
            lines.append(f"  {key:14s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %")
        for fused, base, floor in PAIRS:
            g, m, d = r["ms"][fused], r["ms"][base], r["ms"][floor]
            verdict = "faster, ranges disjoint" if g["max"] < m["min"] else "NOT faster by disjoint ranges"
            lines.append(f"  {fused} / {base}: x{g['median'] / m['median']:6.3f}   {verdict};   against {floor} alone (the old path's floor): x{g['median'] / d['median']:6.3f}")
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
    ap.add_argument("--unsigned", action="store_true", help="unsigned digits instead of balanced ones")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gadget_dot_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.shape:
        return run_point(args.shape, args.terms or 2, args.repeats, not args.unsigned)
    results = []
    for tag in ("cfg2", "cfg3"):
        for terms in TERMS:
            step = f"{tag} terms {terms}"
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", tag, "--terms", str(terms), "--repeats", str(args.repeats)]
            try:
                r = subprocess.run(cmd + (["--unsigned"] if args.unsigned else []), stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
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
