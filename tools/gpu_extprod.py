#!/usr/bin/env python3
"""Same-process A/B of the external product (tn_poly_external_product_prepared_dev, ins = outs = 2) against the two routes a caller
has without it.

  gpu_extprod.py [--out FILE] [--resources FILE] [--repeats N] [--parent-root DIR]   driver: one child process per shape and term count,
                                                                                     each under its own time limit; nothing runs after a
                                                                                     step that failed
  gpu_extprod.py --shape cfg2|cfg3 --terms T [--repeats N] [--baseline-only] [--root DIR]   one point in this process; one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 output rows (base_log 30, 20, 15 for terms 2, 3, 4), cfg3 = n 1024 / 24-bit / 4,096 output
rows (base_log 12, 8, 6): the points of tools/gpu_gadget2.py.  Balanced digits.  A key per row is [rows][2][2][terms][n]; where
that is more than 24 GiB (cfg2, four terms) the per-row point and its baselines run on half the rows, and the report says so.
In one process, after >= 0.15 s of warm launches,
  ext_*      tn_poly_external_product_prepared_dev on a = [rows][2][n]                                          one launch
  a_*        route A: tn_poly_gadget_multidot_prepared_dev (outs = 2) once per input polynomial, the two polynomials held as
             separate contiguous buffers and the key's rows of each input gathered beforehand, then the modular addition of the
             two [rows][2][n] results in torch (an addition and a conditional subtraction of q)               two launches + torch
  a_*_mul    route A's two launches without the addition
  b_*        route B: tn_gadget_decompose_dev on the rows * 2 rows of a, then tn_poly_dot_prepared_dev with 2 * terms terms once
             per component (a set per row: the component's rows gathered beforehand)                             three launches
with * = shared (bhat_sets = 1) and per_set (bhat_sets = rows), are timed interleaved `repeats` times, K rounds per sample
between two events recorded on the stream the kernels run on, and the outputs of the three are compared in full before anything
is timed.  A point is compared with the FASTER of the two routes (by median), the strongest thing a caller can write without the
new call, and counts as faster only where the new call's slowest repeat is below that route's fastest.
--parent-root: a built checkout of the parent commit; at cfg2 / terms 2 route A is timed once more from that library
(--baseline-only --root DIR, a process of its own) and from this library in the same way (--baseline-only), to show that the
kernels this commit measures against are the parent's.
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
INS = 2
STEP_TIMEOUT_S = 240
KEY_LIMIT_BYTES = 24 << 30
KINDS = ("shared", "per_set")


def run_point(tag, terms, repeats, baseline_only, root):
    sys.path.insert(0, root)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED
    plan = engine.Plan(n, q, psi)
    row_bytes = n * plan.elem_bytes
    set_rows = 2 * INS * terms
    rows = {"shared": batch, "per_set": batch if batch * set_rows * row_bytes <= KEY_LIMIT_BYTES else batch // 2}
    a = plan.fill_lcg(batch * INS, 1, 2).reshape(batch, INS, n)                                # [batch][ins][n]
    a_in = [a[:, i].contiguous() for i in range(INS)]                                          # route A: one buffer per input polynomial
    src = plan.fill_lcg(rows["per_set"] * set_rows, 2, 2)
    bhat = plan.prepare(src).tensor                                                            # [rows][2][ins][terms][n]
    del src
    key5 = bhat.reshape(rows["per_set"], 2, INS, terms, n)
    key_in = [key5[:, :, i].contiguous() for i in range(INS)]                                  # route A: [rows][2][terms][n] of input i
    key_out = [key5[:, o].contiguous() for o in range(2)]                                      # route B: [rows][ins * terms][n] of component o
    new = lambda *shape: torch.empty(shape, dtype=a.dtype, device=a.device)
    c = {k: new(rows[k], 2, n) for k in KINDS}
    ra = {k: [new(rows[k], 2, n) for _ in range(INS)] for k in KINDS}
    sa = {k: new(rows[k], 2, n) for k in KINDS}
    ca = {k: new(rows[k], 2, n) for k in KINDS}
    digits = new(batch * INS, terms, n)
    cb = {k: [new(rows[k], n) for _ in range(2)] for k in KINDS}
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    P = lambda t: t.data_ptr()

    def route_a_launches(k):
        sets, r, rc = (1 if k == "shared" else rows[k]), rows[k], 0
        for i in range(INS):      # (input i's rows of ONE set are not contiguous in [2][ins][terms] either: a shared launch takes set 0 of the gathered copy)
            rc |= lib.tn_poly_gadget_multidot_prepared_dev(h, P(a_in[i]), P(key_in[i]), sets, P(ra[k][i]), r, 2, terms, w, flags, st)
        return rc

    def route_a(k):
        rc = route_a_launches(k)
        torch.add(ra[k][0], ra[k][1], out=sa[k])
        torch.where(sa[k] >= q, sa[k] - q, sa[k], out=ca[k])
        return rc

    def route_b(k):
        sets, r = (1 if k == "shared" else rows[k]), rows[k]
        rc = lib.tn_gadget_decompose_dev(h, P(a), P(digits), r * INS, terms, w, flags, st)
        for o in range(2):
            bh = P(bhat) + o * INS * terms * row_bytes if k == "shared" else P(key_out[o])
            rc |= lib.tn_poly_dot_prepared_dev(h, P(digits), bh, sets, P(cb[k][o]), r, INS * terms, st)
        return rc

    def ext(k):
        return lib.tn_poly_external_product_prepared_dev(h, P(a), P(bhat), 1 if k == "shared" else rows[k], P(c[k]), rows[k], INS, 2, terms, w, flags, st)

    launches = {}
    for k in KINDS:
        if not baseline_only:
            launches["ext_" + k] = lambda k=k: ext(k)
        launches["a_" + k] = lambda k=k: route_a(k)
        launches["a_" + k + "_mul"] = lambda k=k: route_a_launches(k)
        if not baseline_only:
            launches["b_" + k] = lambda k=k: route_b(k)
    for fn in launches.values():
        assert fn() == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()
    identical = baseline_only or all(bool(torch.equal(c[k], ca[k])) and bool(torch.equal(c[k][:, 0], cb[k][0])) and bool(torch.equal(c[k][:, 1], cb[k][1]))
                                     for k in KINDS)

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round (one external product, by whichever route)

    est = sample(launches["a_per_set"], 3)
    rounds = max(5, min(500, int(20.0 / est)))    # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for fn in launches.values():
            sample(fn, rounds)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds))
    out = {"shape": name, "tag": tag, "batch": batch, "rows": rows, "terms": terms, "base_log": w, "rounds_per_sample": rounds, "repeats": repeats,
           "identical": identical, "baseline_only": baseline_only, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out["ms"][key] = {"median": med, "min": s[0], "max": s[-1], "spread": (s[-1] - s[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def line(key, m):
    return f"  {key:18s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %"


def report(results, parent, resources):
    lines = ["External product, ins = outs = 2: one tn_poly_external_product_prepared_dev launch against route A (two "
             "tn_poly_gadget_multidot_prepared_dev launches and a modular addition in torch; _mul: the launches alone) and route B "
             "(tn_gadget_decompose_dev, then two tn_poly_dot_prepared_dev launches with 2 * terms terms) (tools/gpu_extprod.py)",
             "A point is compared with the faster route (by median) and counts as faster only where its slowest repeat is below that route's fastest.", ""]
    for r in results:
        lines.append(f"{r['shape']}, terms {r['terms']}, base_log {r['base_log']}, balanced digits   build {r['build_id']}   {r['device']}")
        lines.append(f"  output rows: shared key {r['rows']['shared']}, key per row {r['rows']['per_set']}"
                     + ("" if r["rows"]["per_set"] == r["batch"] else f"   (a key per row for {r['batch']} rows is above 24 GiB: FEWER ROWS at this point)"))
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every word of both components identical to route A and to route B: {r['identical']}")
        for k in KINDS:
            for key in ("ext_" + k, "a_" + k, "a_" + k + "_mul", "b_" + k):
                lines.append(line(key, r["ms"][key]))
        for k in KINDS:
            g, ma, mb = r["ms"]["ext_" + k], r["ms"]["a_" + k], r["ms"]["b_" + k]
            best_name, best = ("route A", ma) if ma["median"] <= mb["median"] else ("route B", mb)
            if g["max"] < best["min"]:
                verdict = "faster, ranges disjoint"
            elif g["min"] > best["max"]:
                verdict = "SLOWER, ranges disjoint"
            else:
                verdict = "WITHIN THE SPREAD"
            lines.append(f"  ext_{k}: x{g['median'] / ma['median']:6.3f} of route A, x{g['median'] / mb['median']:6.3f} of route B; against the faster, {best_name}: "
                         f"x{g['median'] / best['median']:6.3f}   {verdict}")
        lines.append("")
    if parent:
        mine = parent["this"]
        lines.append(f"Baseline soundness: {parent['shape']}, terms {parent['terms']}: route A timed from a library built at the parent commit "
                     f"(build {parent['build_id']}) and from this one (build {mine['build_id']}), each alone in a process of its own in the same job")
        for key in ("a_shared", "a_shared_mul", "a_per_set", "a_per_set_mul"):
            p, m = parent["ms"][key], mine["ms"][key]
            agree = p["min"] <= m["max"] and m["min"] <= p["max"]
            lines.append(line("parent " + key, p))
            lines.append(line("this   " + key, m))
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
    ap.add_argument("--baseline-only", action="store_true", help="time route A alone (a library without the new call)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose tiny_ntt_amd package and library run the point")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit for the baseline-soundness point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extprod_ab.txt"))
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
            if args.parent_root and (tag, terms) == ("cfg2", 2):      # like for like: both libraries time route A alone
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
