#!/usr/bin/env python3
"""Same-process A/B of the two-component gadget product against two launches of the one-component call.

  gpu_gadget2.py [--out FILE] [--resources FILE] [--repeats N] [--parent-root DIR]   driver: one child process per shape and term count,
                                                                                     each under its own time limit; nothing runs after a
                                                                                     step that failed
  gpu_gadget2.py --shape cfg2|cfg3 --terms T [--repeats N] [--baseline-only] [--root DIR]   one point in this process; one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 output rows (base_log 30, 20, 15 for terms 2, 3, 4), cfg3 = n 1024 / 24-bit / 4,096 output
rows (base_log 12, 8, 6): the points of tools/gpu_gadget.py.  Balanced digits.  In one process, after >= 0.15 s of warm launches,
  pair_shared    tn_poly_gadget_multidot_prepared_dev, outs = 2, bhat_sets = 1       one launch
  pair_per_set   the same with bhat_sets = batch
  base_shared    tn_poly_gadget_dot_prepared_dev twice, one launch per component, same a, same prepared rows (bhat_sets = 1)
  base_per_set   the same with bhat_sets = batch (the component's rows gathered beforehand: the one-component call wants them
                 contiguous per output row)
are timed interleaved `repeats` times, K rounds per sample between two events recorded on the stream the kernels run on, and
the outputs are compared in full.  The new call counts as faster only where its slowest repeat is below the baseline's fastest.
--parent-root: a built checkout of the parent commit; at cfg2 / terms 2 the baseline is timed once more from that library
(--baseline-only --root DIR, a process of its own) and from this library in the same way (--baseline-only), to show that the
baseline kernel this commit measures against is the parent's.
--resources appends a file (the resource table, taken where the library was built)."""
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
PAIRS = (("pair_shared", "base_shared"), ("pair_per_set", "base_per_set"))


def run_point(tag, terms, repeats, baseline_only, root):
    sys.path.insert(0, root)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED
    plan = engine.Plan(n, q, psi)
    a = plan.fill_lcg(batch, 1, 2)
    bhat = plan.prepare(plan.fill_lcg(batch * 2 * terms, 2, 2)).tensor                       # [batch][2][terms][n]
    comp = [bhat.reshape(batch, 2, terms, n)[:, o].contiguous() for o in range(2)]          # [batch][terms][n] per component
    c = torch.empty((batch, 2, n), dtype=a.dtype, device=a.device); c2 = torch.empty_like(c)
    cb = [torch.empty((batch, n), dtype=a.dtype, device=a.device) for _ in range(4)]
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    pa, ph, pc, pc2 = (t.data_ptr() for t in (a, bhat, c, c2))
    pcomp, pcb = [t.data_ptr() for t in comp], [t.data_ptr() for t in cb]
    row_bytes = n * plan.elem_bytes

    def one(bh, sets, out):
        return lib.tn_poly_gadget_dot_prepared_dev(h, pa, bh, sets, out, batch, terms, w, flags, st)

    launches = {
        "base_shared": lambda: one(ph, 1, pcb[0]) | one(ph + terms * row_bytes, 1, pcb[1]),
        "base_per_set": lambda: one(pcomp[0], batch, pcb[2]) | one(pcomp[1], batch, pcb[3]),
    }
    if not baseline_only:
        launches["pair_shared"] = lambda: lib.tn_poly_gadget_multidot_prepared_dev(h, pa, ph, 1, pc, batch, 2, terms, w, flags, st)
        launches["pair_per_set"] = lambda: lib.tn_poly_gadget_multidot_prepared_dev(h, pa, ph, batch, pc2, batch, 2, terms, w, flags, st)
    for fn in launches.values():
        assert fn() == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()
    identical = baseline_only or all(bool(torch.equal(x, y)) for x, y in ((c[:, 0], cb[0]), (c[:, 1], cb[1]), (c2[:, 0], cb[2]), (c2[:, 1], cb[3])))

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round (one launch of the pair, or two launches)

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
    out = {"shape": name, "tag": tag, "batch": batch, "terms": terms, "base_log": w, "rounds_per_sample": rounds, "repeats": repeats,
           "identical": identical, "baseline_only": baseline_only, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out["ms"][key] = {"median": med, "min": s[0], "max": s[-1], "spread": (s[-1] - s[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def line(key, m):
    return f"  {key:14s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %"


def report(results, parent, resources):
    lines = ["Gadget product, two components: one tn_poly_gadget_multidot_prepared_dev launch (outs = 2) against two tn_poly_gadget_dot_prepared_dev "
             "launches (tools/gpu_gadget2.py)", ""]
    for r in results:
        lines.append(f"{r['shape']}, {r['batch']} output rows, terms {r['terms']}, base_log {r['base_log']}, balanced digits   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every word of both components identical to the two launches: {r['identical']}")
        for key in ("pair_shared", "base_shared", "pair_per_set", "base_per_set"):
            lines.append(line(key, r["ms"][key]))
        for pair, base in PAIRS:
            g, m = r["ms"][pair], r["ms"][base]
            verdict = "faster, ranges disjoint" if g["max"] < m["min"] else "NOT faster by disjoint ranges"
            lines.append(f"  {pair} / {base}: x{g['median'] / m['median']:6.3f}   {verdict}")
        lines.append("")
    if parent:
        mine = parent["this"]
        lines.append(f"Baseline soundness: {parent['shape']}, terms {parent['terms']}: the two one-component launches timed from a library built at the parent commit "
                     f"(build {parent['build_id']}) and from this one (build {mine['build_id']}), each alone in a process of its own in the same job")
        for key in ("base_shared", "base_per_set"):
            p, m = parent["ms"][key], mine["ms"][key]
            agree = p["min"] <= m["max"] and m["min"] <= p["max"]
            lines.append(line("parent " + key[5:], p))
            lines.append(line("this   " + key[5:], m))
            lines.append(f"  medians x{m['median'] / p['median']:6.3f}; ranges {'overlap' if agree else 'DO NOT overlap'}")
        lines.append("")
    if resources:
        with open(resources) as f:
            lines.append(f.read().rstrip())
        lines.append("")
    return "\n".join(lines)


def child(args, extra, step):
    cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats)] + extra
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        print(f"{step}: no result within {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
        return 124, None
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        print(f"{step}: exit status {r.returncode}; stopping", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--terms", type=int, choices=TERMS)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--baseline-only", action="store_true", help="time the two one-component launches alone (a library without the new call)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose tiny_ntt_amd package and library run the point")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit for the baseline-soundness point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gadget_pair_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.shape:
        return run_point(args.shape, args.terms or 2, args.repeats, args.baseline_only, os.path.abspath(args.root))
    results, parent = [], None
    for tag in ("cfg2", "cfg3"):
        for terms in TERMS:
            rc, res = child(args, ["--shape", tag, "--terms", str(terms)], f"{tag} terms {terms}")
            if rc:
                return rc
            results.append(res)
            if args.parent_root and (tag, terms) == ("cfg2", 2):      # like for like: both libraries time the baseline alone
                rc, parent = child(args, ["--shape", tag, "--terms", str(terms), "--baseline-only", "--root", args.parent_root], "parent baseline")
                if rc:
                    return rc
                rc, alone = child(args, ["--shape", tag, "--terms", str(terms), "--baseline-only"], "this baseline")
                if rc:
                    return rc
                parent["this"] = alone
    text = report(results, parent, args.resources)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
