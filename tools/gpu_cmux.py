#!/usr/bin/env python3
"""Same-process A/B of the CMux rotation step (tn_poly_cmux_rotate_prepared_dev) against the explicit route a caller has without it.

  gpu_cmux.py [--out FILE] [--resources FILE] [--repeats N]     driver: one child process per shape and term count, each under its
                                                                own time limit; nothing runs after a step that failed
  gpu_cmux.py --shape cfg2|cfg3 --terms T [--repeats N]         one point in this process; one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 rows (base_log 30, 20, 15 for terms 2, 3, 4), cfg3 = n 1024 / 24-bit / 4,096 rows
(base_log 12, 8, 6): the points of tools/gpu_extprod.py.  Balanced digits, random exponents (any 32-bit word).  A key per row is
[rows][2][2][terms][n]; where that is more than 24 GiB (cfg2, four terms) the per-row point and its baselines run on half the
rows, and the report says so.  a holds canonical residues, so that the route's addition is the plain torch one.
In one process, after >= 0.15 s of warm launches,
  cmux_*       tn_poly_cmux_rotate_prepared_dev on a = [rows][2][n]                                              one launch
  route_*      the explicit route: tn_monomial_mul_dev (group 2, TN_MONOMIAL_MINUS_ONE), tn_poly_external_product_prepared_dev
               (ins = outs = 2) on its output, then the addition of a in torch (an addition, a comparison, a subtraction of q
               and a select)                                                                                     two launches + torch
  route_*_mul  the same route's two library launches without the addition
  ext_*        a plain tn_poly_external_product_prepared_dev launch on the same rows of a: what the rotation and the add-in cost
               on top of the product (one more read of a by count, and a second read of the same row)
with * = shared (bhat_sets = 1) and per_set (bhat_sets = rows), are timed interleaved `repeats` times, K rounds per sample between
two events recorded on the stream the kernels run on; the outputs of the one launch and of the route are compared in full before
anything is timed.  A point counts as faster only where the new call's slowest repeat is below the route's fastest.
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
KEY_LIMIT_BYTES = 24 << 30
KINDS = ("shared", "per_set")


def run_point(tag, terms, repeats):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED
    plan = engine.Plan(n, q, psi)
    row_bytes = n * plan.elem_bytes
    set_rows = 4 * terms
    rows = {"shared": batch, "per_set": batch if batch * set_rows * row_bytes <= KEY_LIMIT_BYTES else batch // 2}
    a = plan.automorphism(plan.fill_lcg(batch * 2, 1, 2), 1).reshape(batch, 2, n)               # [batch][2][n], canonical residues
    exps = torch.from_numpy(np.random.default_rng(17).integers(0, 2 ** 32, batch, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(a.device)
    src = plan.fill_lcg(rows["per_set"] * set_rows, 2, 2)
    bhat = plan.prepare(src).tensor                                                            # [rows][2][2][terms][n]
    del src
    new = lambda *shape: torch.empty(shape, dtype=a.dtype, device=a.device)
    c = {k: new(rows[k], 2, n) for k in KINDS}
    m, p, s, cr = new(batch, 2, n), new(batch, 2, n), new(batch, 2, n), {k: new(rows[k], 2, n) for k in KINDS}
    pe = new(batch, 2, n)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    P = lambda t: t.data_ptr()
    sets = lambda k: 1 if k == "shared" else rows[k]

    def route_launches(k):
        r = rows[k]
        rc = lib.tn_monomial_mul_dev(h, P(a), P(exps), P(m), r, 2, engine.MONOMIAL_MINUS_ONE, st)
        return rc | lib.tn_poly_external_product_prepared_dev(h, P(m), P(bhat), sets(k), P(p), r, 2, 2, terms, w, flags, st)

    def route(k):
        r = rows[k]
        rc = route_launches(k)
        torch.add(a[:r], p[:r], out=s[:r])
        torch.where(s[:r] >= q, s[:r] - q, s[:r], out=cr[k])
        return rc

    def cmux(k):
        return lib.tn_poly_cmux_rotate_prepared_dev(h, P(a), P(exps), P(bhat), sets(k), P(c[k]), rows[k], 2, terms, w, flags, st)

    def ext(k):
        return lib.tn_poly_external_product_prepared_dev(h, P(a), P(bhat), sets(k), P(pe), rows[k], 2, 2, terms, w, flags, st)

    launches = {}
    for k in KINDS:
        launches["cmux_" + k] = lambda k=k: cmux(k)
        launches["route_" + k] = lambda k=k: route(k)
        launches["route_" + k + "_mul"] = lambda k=k: route_launches(k)
        launches["ext_" + k] = lambda k=k: ext(k)
    for fn in launches.values():
        assert fn() == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()
    identical = all(bool(torch.equal(c[k], cr[k])) for k in KINDS)

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round (one step, by whichever route)

    est = sample(launches["route_per_set"], 3)
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
           "identical": identical, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        srt = sorted(v)
        med = srt[len(srt) // 2]
        out["ms"][key] = {"median": med, "min": srt[0], "max": srt[-1], "spread": (srt[-1] - srt[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def line(key, m):
    return f"  {key:20s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %"


def verdict(g, base):
    if g["max"] < base["min"]:
        return "faster, ranges disjoint"
    if g["min"] > base["max"]:
        return "SLOWER, ranges disjoint"
    return "WITHIN THE SPREAD"


def report(results, resources):
    lines = ["CMux rotation step: one tn_poly_cmux_rotate_prepared_dev launch against the explicit route (tn_monomial_mul_dev with "
             "TN_MONOMIAL_MINUS_ONE, tn_poly_external_product_prepared_dev, the addition of a in torch; _mul: the two launches alone) and "
             "against a plain tn_poly_external_product_prepared_dev launch on the same rows (tools/gpu_cmux.py)",
             "A point counts as faster only where the new call's slowest repeat is below the other's fastest.", ""]
    for r in results:
        lines.append(f"{r['shape']}, terms {r['terms']}, base_log {r['base_log']}, balanced digits, random exponents   build {r['build_id']}   {r['device']}")
        lines.append(f"  rows: shared key {r['rows']['shared']}, key per row {r['rows']['per_set']}"
                     + ("" if r["rows"]["per_set"] == r["batch"] else f"   (a key per row for {r['batch']} rows is above 24 GiB: FEWER ROWS at this point)"))
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every word identical to the explicit route: {r['identical']}")
        for k in KINDS:
            for key in ("cmux_" + k, "route_" + k, "route_" + k + "_mul", "ext_" + k):
                lines.append(line(key, r["ms"][key]))
        for k in KINDS:
            g, full, mul, e = (r["ms"][key] for key in ("cmux_" + k, "route_" + k, "route_" + k + "_mul", "ext_" + k))
            lines.append(f"  cmux_{k}: x{g['median'] / full['median']:6.3f} of the route ({verdict(g, full)}); x{g['median'] / mul['median']:6.3f} of its two "
                         f"launches ({verdict(g, mul)}); x{g['median'] / e['median']:6.3f} of the plain external product ({verdict(g, e)})")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmux_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.shape:
        return run_point(args.shape, args.terms or 2, args.repeats)
    results = []
    for tag in ("cfg2", "cfg3"):
        for terms in TERMS:
            rc, res = child(args, ["--shape", tag, "--terms", str(terms)], f"{tag} terms {terms}")
            if rc:
                return rc
            results.append(res)
    text = report(results, args.resources)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
