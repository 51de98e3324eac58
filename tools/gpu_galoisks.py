#!/usr/bin/env python3
"""Same-process A/B of the automorphism key switch (tn_poly_galois_keyswitch_prepared_dev) against the explicit route a caller has without it.

  gpu_galoisks.py [--out FILE] [--resources FILE] [--repeats N]     driver: one child process per shape and term count, each under
                                                                    its own time limit; nothing runs after a step that failed
  gpu_galoisks.py --shape cfg2|cfg3 --terms T [--repeats N]         one point in this process; one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 rows (base_log 30, 20, 15 for terms 2, 3, 4), cfg3 = n 1024 / 24-bit / 4,096 rows
(base_log 12, 8, 6): the points of tools/gpu_cmux.py.  Balanced digits; g in {3, 5, 2n - 1, one seeded}, every series once per g.
A key per row is [rows][2][terms][n]; where that is more than 24 GiB the per-row point and its baselines run on half the rows, and
the report says so.  a holds canonical residues, so that the route's addition is the plain torch one.  The one launch reads
a = [rows][2][n]; the route reads the same words in the layout that suits IT best, [2][rows][n], so that the rotated second
components are the contiguous rows the multidot call takes and no copy is part of the route.
In one process, after >= 0.15 s of warm launches,
  ks_*_g        tn_poly_galois_keyswitch_prepared_dev on a = [rows][2][n]                                         one launch
  route_*_g     the explicit route: tn_automorphism_dev on the 2 * rows rows (count 1), tn_poly_gadget_multidot_prepared_dev
                (outs 2) on the rotated second components, then the addition of the rotated first components to component 0 in
                torch (an addition, a comparison, a subtraction of q and a select)                                  two launches + torch
  route_*_g_mul the same route's two library launches without the addition
  plain_*       a plain tn_poly_gadget_multidot_prepared_dev launch (outs 2) on the unrotated second components: what the two
                permutations, their barriers and the second input row cost on top of the key switch
with * = shared (bhat_sets = 1) and per_set (bhat_sets = rows), are timed interleaved `repeats` times, K rounds per sample between
two events recorded on the stream the kernels run on; for every g the outputs of the one launch and of the route are compared in
full before anything is timed.  A point counts as faster only where the new call's slowest repeat is below the other's fastest.
--resources appends a file (the resource table, taken where the library was built)."""
import argparse
import ctypes
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
STEP_TIMEOUT_S = 300
KEY_LIMIT_BYTES = 24 << 30
KINDS = ("shared", "per_set")


def galois_elements(n):
    import numpy as np
    return [3, 5, 2 * n - 1, int(np.random.default_rng(17).integers(0, 2 * n)) | 1]


def run_point(tag, terms, repeats):
    sys.path.insert(0, ROOT)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED
    plan = engine.Plan(n, q, psi)
    row_bytes = n * plan.elem_bytes
    set_rows = 2 * terms
    rows = {"shared": batch, "per_set": batch if batch * set_rows * row_bytes <= KEY_LIMIT_BYTES else batch // 2}
    gs = galois_elements(n)
    a = plan.automorphism(plan.fill_lcg(batch * 2, 1, 2), 1).reshape(batch, 2, n)               # [batch][2][n], canonical residues
    planar = a.transpose(0, 1).contiguous()                                                    # [2][batch][n]: the route's layout
    src = plan.fill_lcg(rows["per_set"] * set_rows, 2, 2)
    bhat = plan.prepare(src).tensor                                                            # [rows][2][terms][n]
    del src
    new = lambda *shape: torch.empty(shape, dtype=a.dtype, device=a.device)
    c = {k: new(rows[k], 2, n) for k in KINDS}
    rot, s, cr, pe = new(2, batch, n), new(batch, n), {k: new(rows[k], 2, n) for k in KINDS}, new(batch, 2, n)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    P = lambda t: t.data_ptr()
    sets = lambda k: 1 if k == "shared" else rows[k]
    one = {g: (ctypes.c_uint32 * 1)(g) for g in gs}

    def route_launches(k, g):
        r = rows[k]
        # (fewer rows than batch: the two components separately, so that each stays the first r rows of its plane)
        if r == batch:
            rc = lib.tn_automorphism_dev(h, P(planar), P(rot), 2 * batch, one[g], 1, st)
        else:
            rc = lib.tn_automorphism_dev(h, P(planar[0]), P(rot[0]), r, one[g], 1, st) | lib.tn_automorphism_dev(h, P(planar[1]), P(rot[1]), r, one[g], 1, st)
        return rc | lib.tn_poly_gadget_multidot_prepared_dev(h, P(rot[1]), P(bhat), sets(k), P(cr[k]), r, 2, terms, w, flags, st)

    def route(k, g):
        r = rows[k]
        rc = route_launches(k, g)
        torch.add(rot[0, :r], cr[k][:, 0], out=s[:r])
        torch.where(s[:r] >= q, s[:r] - q, s[:r], out=cr[k][:, 0])
        return rc

    def ks(k, g):
        return lib.tn_poly_galois_keyswitch_prepared_dev(h, P(a), g, P(bhat), sets(k), P(c[k]), rows[k], terms, w, flags, st)

    def plain(k):
        return lib.tn_poly_gadget_multidot_prepared_dev(h, P(planar[1]), P(bhat), sets(k), P(pe), rows[k], 2, terms, w, flags, st)

    launches = {}
    identical = True
    for k in KINDS:
        for g in gs:
            launches[f"ks_{k}_{g}"] = lambda k=k, g=g: ks(k, g)
            launches[f"route_{k}_{g}"] = lambda k=k, g=g: route(k, g)
            launches[f"route_{k}_{g}_mul"] = lambda k=k, g=g: route_launches(k, g)
            for key in (f"ks_{k}_{g}", f"route_{k}_{g}"):
                assert launches[key]() == engine.TN_OK, lib.tn_last_error().decode()
            torch.cuda.synchronize()
            identical = identical and bool(torch.equal(c[k], cr[k]))
        launches["plain_" + k] = lambda k=k: plain(k)
        assert plain(k) == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round (one key switch, by whichever route)

    est = sample(launches[f"route_per_set_{gs[0]}"], 3)
    rounds = max(3, min(200, int(10.0 / est)))    # ~10 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for fn in launches.values():
            sample(fn, rounds)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds))
    out = {"shape": name, "tag": tag, "batch": batch, "rows": rows, "terms": terms, "base_log": w, "rounds_per_sample": rounds, "repeats": repeats,
           "galois": gs, "identical": identical, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        srt = sorted(v)
        med = srt[len(srt) // 2]
        out["ms"][key] = {"median": med, "min": srt[0], "max": srt[-1], "spread": (srt[-1] - srt[0]) / med}
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def line(key, m):
    return f"  {key:28s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %"


def verdict(g, base):
    if g["max"] < base["min"]:
        return "faster, ranges disjoint"
    if g["min"] > base["max"]:
        return "SLOWER, ranges disjoint"
    return "WITHIN THE SPREAD"


def span(values):
    return f"x{min(values):6.3f} -{max(values):6.3f}"


def verdicts(pairs):
    v = sorted({verdict(g, base) for g, base in pairs})
    return v[0] + " for every g" if len(v) == 1 else "MIXED over g: " + "; ".join(v)


def report(results, resources):
    lines = ["Automorphism key switch: one tn_poly_galois_keyswitch_prepared_dev launch against the explicit route (tn_automorphism_dev on both "
             "components, tn_poly_gadget_multidot_prepared_dev with outs 2 on the rotated second ones, the addition in torch; _mul: the two "
             "launches alone) and against a plain tn_poly_gadget_multidot_prepared_dev launch on the unrotated second components "
             "(tools/gpu_galoisks.py)",
             "The route reads the same words as [2][rows][n], the layout in which it needs no copy; the one launch reads [rows][2][n].",
             "A point counts as faster only where the new call's slowest repeat is below the other's fastest.  Ratios are of medians, "
             "given as the range over the four Galois elements.", ""]
    for r in results:
        gs = r["galois"]
        lines.append(f"{r['shape']}, terms {r['terms']}, base_log {r['base_log']}, balanced digits, g in {gs}   build {r['build_id']}   {r['device']}")
        lines.append(f"  rows: shared key {r['rows']['shared']}, key per row {r['rows']['per_set']}"
                     + ("" if r["rows"]["per_set"] == r["batch"] else f"   (a key per row for {r['batch']} rows is above 24 GiB: FEWER ROWS at this point)"))
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every word identical to the explicit route for every g: {r['identical']}")
        for k in KINDS:
            for g in gs:
                for key in (f"ks_{k}_{g}", f"route_{k}_{g}", f"route_{k}_{g}_mul"):
                    lines.append(line(key, r["ms"][key]))
            lines.append(line("plain_" + k, r["ms"]["plain_" + k]))
        for k in KINDS:
            m = r["ms"]
            new = [m[f"ks_{k}_{g}"] for g in gs]
            full = [m[f"route_{k}_{g}"] for g in gs]
            mul = [m[f"route_{k}_{g}_mul"] for g in gs]
            e = m["plain_" + k]
            lines.append(f"  ks_{k}: {min(x['median'] for x in new) * 1e3:.1f} - {max(x['median'] for x in new) * 1e3:.1f} us over g; "
                         f"{span([x['median'] / y['median'] for x, y in zip(new, full)])} of the route ({verdicts(list(zip(new, full)))}); "
                         f"{span([x['median'] / y['median'] for x, y in zip(new, mul)])} of its two launches ({verdicts(list(zip(new, mul)))}); "
                         f"{span([x['median'] / e['median'] for x in new])} of the plain key switch ({verdicts([(x, e) for x in new])})")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "galoisks_ab.txt"))
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
