#!/usr/bin/env python3
"""Same-process A/B of the pack / trace step (tn_poly_pack_step_prepared_dev) against the explicit route a caller has without it.

  gpu_pack.py [--out FILE] [--resources FILE] [--repeats N]     driver: one child process per shape and term count, each under
                                                                its own time limit; nothing runs after a step that failed
  gpu_pack.py --shape cfg2|cfg3 --terms T [--repeats N]         one point in this process; one JSON line

Shapes: cfg2 = n 4096 / 60-bit / 65,536 rows (base_log 30, 20, 15 for terms 2, 3, 4), cfg3 = n 1024 / 24-bit / 4,096 rows
(base_log 12, 8, 6): the points of tools/gpu_galoisks.py.  Balanced digits, one shared key; g in {3, 5, one seeded}, rot = n / 2,
n / 4 and one seeded with them; every series once per g.  ev and od hold canonical residues, so that the route's passes are the
plain torch ones.  In one process, after >= 0.15 s of warm launches,
  pack_g        tn_poly_pack_step_prepared_dev on ev, od = [rows][2][n]                                              one launch
  route_g       the explicit route: tn_monomial_mul_dev on od (exponent rot for every row, group 2); s = ev + t and d = ev - t
                mod q in torch (an addition or subtraction, a comparison, a correction and a select each);
                tn_poly_galois_keyswitch_prepared_dev on d; the addition of s mod q in torch                          two launches + torch
  route_g_mul   the same route's two library launches without the torch passes
  ks_g          a plain tn_poly_galois_keyswitch_prepared_dev on ev: what the second input ciphertext and the sums cost on top
  trace_g       the trace step: tn_poly_pack_step_prepared_dev with od == NULL
  trace_route_g its route: the key switch of ev and the addition of ev mod q in torch
are timed interleaved `repeats` times, K rounds per sample between two events recorded on the stream the kernels run on; for every
g the outputs of the one launch and of the route are compared in full before anything is timed (pack and trace form).  At cfg3
also one whole Plan.pack_lwes (n = 1024, groups 64, count 1024 and count 32, random keys of log2 n levels) against the same tree
built from the route's calls through the Python package, outputs compared first; both sides allocate their temporaries.
A point counts as faster only where the new call's slowest repeat is below the other's fastest.
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
STEP_TIMEOUT_S = 300
TREE_GROUPS, TREE_COUNTS = 64, (1024, 32)


def elements(n):
    import numpy as np
    rng = np.random.default_rng(17)
    return [(3, n // 2), (5, n // 4), (int(rng.integers(0, 2 * n)) | 1, int(rng.integers(0, 2 * n)))]


def run_point(tag, terms, repeats):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from tiny_ntt_amd import engine, numtheory
    name, n, q, psi, batch, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED
    plan = engine.Plan(n, q, psi)
    pairs = elements(n)
    ev = plan.automorphism(plan.fill_lcg(batch * 2, 1, 2), 1).reshape(batch, 2, n)               # canonical residues
    od = plan.automorphism(plan.fill_lcg(batch * 2, 7, 2), 1).reshape(batch, 2, n)
    bhat = plan.prepare(plan.fill_lcg(2 * terms, 2, 2)).tensor                                    # one shared key
    new = lambda: torch.empty((batch, 2, n), dtype=ev.dtype, device=ev.device)
    c, cr, t, s, d, tmp, pk = new(), new(), new(), new(), new(), new(), new()
    exps = {rot: torch.full((batch,), rot, dtype=torch.int32, device=ev.device) for _, rot in pairs}
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    P = lambda x: x.data_ptr()

    def add_mod(x, y, out):
        torch.add(x, y, out=tmp)
        torch.where(tmp >= q, tmp - q, tmp, out=out)

    def sub_mod(x, y, out):
        torch.sub(x, y, out=tmp)
        torch.where(tmp < 0, tmp + q, tmp, out=out)

    def route_launches(g, rot):
        return lib.tn_monomial_mul_dev(h, P(od), P(exps[rot]), P(t), batch, 2, 0, st) | \
            lib.tn_poly_galois_keyswitch_prepared_dev(h, P(d), g, P(bhat), 1, P(cr), batch, terms, w, flags, st)

    def route(g, rot):
        rc = lib.tn_monomial_mul_dev(h, P(od), P(exps[rot]), P(t), batch, 2, 0, st)
        add_mod(ev, t, s)
        sub_mod(ev, t, d)
        rc |= lib.tn_poly_galois_keyswitch_prepared_dev(h, P(d), g, P(bhat), 1, P(cr), batch, terms, w, flags, st)
        add_mod(cr, s, cr)
        return rc

    def pack(g, rot):
        return lib.tn_poly_pack_step_prepared_dev(h, P(ev), P(od), rot, g, P(bhat), 1, P(c), batch, terms, w, flags, st)

    def ks(g):
        return lib.tn_poly_galois_keyswitch_prepared_dev(h, P(ev), g, P(bhat), 1, P(pk), batch, terms, w, flags, st)

    def trace(g):
        return lib.tn_poly_pack_step_prepared_dev(h, P(ev), None, 0, g, P(bhat), 1, P(c), batch, terms, w, flags, st)

    def trace_route(g):
        rc = lib.tn_poly_galois_keyswitch_prepared_dev(h, P(ev), g, P(bhat), 1, P(cr), batch, terms, w, flags, st)
        add_mod(cr, ev, cr)
        return rc

    launches = {}
    identical = True
    for g, rot in pairs:
        launches[f"pack_{g}"] = lambda g=g, rot=rot: pack(g, rot)
        launches[f"route_{g}"] = lambda g=g, rot=rot: route(g, rot)
        launches[f"route_{g}_mul"] = lambda g=g, rot=rot: route_launches(g, rot)
        launches[f"ks_{g}"] = lambda g=g: ks(g)
        launches[f"trace_{g}"] = lambda g=g: trace(g)
        launches[f"trace_route_{g}"] = lambda g=g: trace_route(g)
        for one, other in ((f"trace_{g}", f"trace_route_{g}"), (f"pack_{g}", f"route_{g}")):
            assert launches[one]() == engine.TN_OK and launches[other]() == engine.TN_OK, lib.tn_last_error().decode()
            torch.cuda.synchronize()
            identical = identical and bool(torch.equal(c, cr))
        assert ks(g) == engine.TN_OK, lib.tn_last_error().decode()
    torch.cuda.synchronize()

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round

    def measure(fns, est_key):
        est = sample(fns[est_key], 3)
        rounds = max(3, min(200, int(10.0 / est)))    # ~10 ms of launches per sample
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
            for fn in fns.values():
                sample(fn, rounds)
        times = {key: [] for key in fns}
        for _ in range(repeats):
            for key, fn in fns.items():
                times[key].append(sample(fn, rounds))
        ms = {}
        for key, v in times.items():
            srt = sorted(v)
            med = srt[len(srt) // 2]
            ms[key] = {"median": med, "min": srt[0], "max": srt[-1], "spread": (srt[-1] - srt[0]) / med}
        return ms, rounds

    ms, rounds = measure(launches, f"route_{pairs[0][0]}")
    out = {"shape": name, "tag": tag, "batch": batch, "terms": terms, "base_log": w, "rounds_per_sample": rounds, "repeats": repeats,
           "pairs": pairs, "identical": identical, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": ms}

    if tag == "cfg3":                                 # one whole packing tree through the Python package
        del c, cr, t, s, d, tmp, pk
        levels = numtheory.pack_elements(n)
        key_rows = 2 * terms
        keys = plan.prepare(plan.fill_lcg(len(levels) * key_rows, 3, 2))

        def step_route(e, o, rot, g, key):
            tt = plan.monomial_mul(o, exps_tree[(rot, int(e.shape[0]))]) if o is not None else None
            ss = e + tt if o is not None else e
            ss = torch.where(ss >= q, ss - q, ss) if o is not None else ss
            dd = e - tt if o is not None else e
            dd = torch.where(dd < 0, dd + q, dd) if o is not None else dd
            r = plan.poly_galois_keyswitch_prepared(dd, g, key, terms, w, True) + ss
            return torch.where(r >= q, r - q, r)

        def tree_route(lwe):
            groups, count = int(lwe.shape[0]), int(lwe.shape[1])
            cur = plan.lwe_embed(lwe.transpose(0, 1).contiguous().reshape(count * groups, n + 1), 0)
            for lv, (k, g) in enumerate(levels, start=1):
                key = engine.PreparedOperand(plan, keys.tensor[(lv - 1) * key_rows:lv * key_rows], key_rows)
                r = int(cur.shape[0])
                cur = step_route(cur[:r // 2], cur[r // 2:], k, g, key) if r > groups else step_route(cur, None, 0, g, key)
            return cur

        exps_tree, tree, tree_same = {}, {}, True
        for count in TREE_COUNTS:
            r = count * TREE_GROUPS
            for lv, (k, g) in enumerate(levels, start=1):
                if r > TREE_GROUPS:
                    r //= 2
                    exps_tree[(k, r)] = torch.full((r,), k, dtype=torch.int32, device=ev.device)
            words = TREE_GROUPS * count * (n + 1)
            lwe = plan.fill_lcg(-(-words // n), 5, 2).reshape(-1)[:words].reshape(TREE_GROUPS, count, n + 1).contiguous()
            fused = plan.pack_lwes(lwe, keys, terms, w, True)
            tree_same = tree_same and bool(torch.equal(fused, tree_route(lwe)))
            fns = {f"tree_{count}": lambda lwe=lwe: (plan.pack_lwes(lwe, keys, terms, w, True), engine.TN_OK)[1],
                   f"tree_route_{count}": lambda lwe=lwe: (tree_route(lwe), engine.TN_OK)[1]}
            tms, _ = measure(fns, f"tree_route_{count}")
            tree.update(tms)
        out["tree"], out["tree_identical"], out["tree_groups"] = tree, tree_same, TREE_GROUPS
        identical = identical and tree_same
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
    lines = ["Pack / trace step: one tn_poly_pack_step_prepared_dev launch against the explicit route (tn_monomial_mul_dev on od, the sum and "
             "the difference mod q in torch, tn_poly_galois_keyswitch_prepared_dev on the difference, the addition of the sum in torch; _mul: "
             "the two launches alone), against a plain tn_poly_galois_keyswitch_prepared_dev on ev, and the trace step (od == NULL) against "
             "its route (the key switch of ev, the addition in torch) (tools/gpu_pack.py)",
             "A point counts as faster only where the new call's slowest repeat is below the other's fastest.  Ratios are of medians, "
             "given as the range over the three (g, rot) pairs.  One shared key, balanced digits.", ""]
    for r in results:
        gs = [g for g, _ in r["pairs"]]
        lines.append(f"{r['shape']}, {r['batch']} rows, terms {r['terms']}, base_log {r['base_log']}, (g, rot) in {r['pairs']}   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every word identical to the explicit route for every g, "
                     f"pack and trace form: {r['identical']}")
        m = r["ms"]
        for g in gs:
            for key in (f"pack_{g}", f"route_{g}", f"route_{g}_mul", f"ks_{g}", f"trace_{g}", f"trace_route_{g}"):
                lines.append(line(key, m[key]))
        new, full, mul = [m[f"pack_{g}"] for g in gs], [m[f"route_{g}"] for g in gs], [m[f"route_{g}_mul"] for g in gs]
        plain, tr, trr = [m[f"ks_{g}"] for g in gs], [m[f"trace_{g}"] for g in gs], [m[f"trace_route_{g}"] for g in gs]
        ratio = lambda xs, ys: span([x["median"] / y["median"] for x, y in zip(xs, ys)])
        lines.append(f"  pack: {min(x['median'] for x in new) * 1e3:.1f} - {max(x['median'] for x in new) * 1e3:.1f} us over g; "
                     f"{ratio(new, full)} of the route ({verdicts(list(zip(new, full)))}); "
                     f"{ratio(new, mul)} of its two launches ({verdicts(list(zip(new, mul)))}); "
                     f"{ratio(new, plain)} of the plain key switch ({verdicts(list(zip(new, plain)))})")
        lines.append(f"  trace: {min(x['median'] for x in tr) * 1e3:.1f} - {max(x['median'] for x in tr) * 1e3:.1f} us over g; "
                     f"{ratio(tr, trr)} of its route ({verdicts(list(zip(tr, trr)))}); "
                     f"{ratio(tr, plain)} of the plain key switch ({verdicts(list(zip(tr, plain)))})")
        if "tree" in r:
            lines.append(f"  Plan.pack_lwes, groups {r['tree_groups']}, against the route-built tree (both through the Python package, temporaries allocated "
                         f"on both sides); outputs identical: {r['tree_identical']}")
            for count in TREE_COUNTS:
                a, b = r["tree"][f"tree_{count}"], r["tree"][f"tree_route_{count}"]
                lines.append(line(f"tree_{count}", a))
                lines.append(line(f"tree_route_{count}", b))
                lines.append(f"  count {count}: x{a['median'] / b['median']:6.3f} of the route-built tree ({verdict(a, b)})")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_ab.txt"))
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
