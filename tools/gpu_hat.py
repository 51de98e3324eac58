#!/usr/bin/env python3
"""Same-process A/B of the transform-domain entry points (tn_poly_dot_hat_dev, tn_unprepare_dev) against the best way to get
the same bits without them.

  gpu_hat.py [--out FILE] [--resources FILE] [--repeats N]       driver: one child process per point, each under its own time
                                                                 limit; nothing runs after a step that failed
  gpu_hat.py --point matvec|term|unprep --shape cfg2|cfg3 [--size K] [--repeats N]      one point in this process; one JSON line

Shapes: cfg2 = n 4096 / 60-bit, cfg3 = n 1024 / 24-bit.  Points:
  matvec  c[i] = sum_j A[i][j] * s[j], k = l = --size (2, 4), A prepared ahead of time, over 16,384 (cfg2) / 4,096 (cfg3) vectors:
            new   one tn_prepare_dev of the vectors' B * l rows, then k launches of tn_poly_dot_hat_dev against a shared set
            base  k launches of tn_poly_dot_prepared_dev against a shared set, on the un-prepared vectors
          the prepare is inside the timed region; the two paths' outputs are compared in full
  term    terms = --size (2, 3, 4), 65,536 (cfg2) / 4,096 (cfg3) output rows, a already prepared for the new call:
            hat_shared / hat_per_set      one tn_poly_dot_hat_dev launch, coefficients out
            kept_shared / kept_per_set    the same with out_prepared = 1 (no transform)
            dot_shared / dot_per_set      one tn_poly_dot_prepared_dev launch on the un-prepared a: the baseline
          with the bytes each launch moves per second beside a device-to-device copy of one operand measured in the same process
  unprep  tn_unprepare_dev against tn_prepare_dev and tn_ntt_inverse_dev at the same row count (65,536 / 4,096): the same traffic
Every measurement: after >= 0.15 s of warm launches, `repeats` interleaved samples of K rounds each between two events on the
stream the kernels run on; median, min, max and the spread (max - min) / median.  The new path counts as faster only where its
max is below the baseline's min (disjoint ranges).  --resources appends a file (the resource table of the new kernels and the
diff of the existing kernels' report against the parent commit, taken where the library was built) to the report."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name, n, q, psi, output rows of the term / unprep points, vectors of the matvec point
SHAPES = {
    "cfg2": ("n=4096 60-bit", 4096, 1152921504606830593, 431606828070683274, 65536, 16384),
    "cfg3": ("n=1024 24-bit", 1024, 8380417, 5548360, 4096, 4096),
}
POINTS = [("matvec", 2), ("matvec", 4), ("term", 2), ("term", 3), ("term", 4), ("unprep", 0)]
STEP_TIMEOUT_S = 240
# (new, baseline) pairs judged by disjoint ranges
PAIRS = {
    "matvec": (("new", "base"),),
    "term": (("hat_shared", "dot_shared"), ("hat_per_set", "dot_per_set"), ("kept_shared", "dot_shared"), ("kept_per_set", "dot_per_set")),
    "unprep": (("unprepare", "prepare"), ("unprepare", "ntt_inverse")),
}


def measure(torch, engine, lib, launches, repeats, pilot):
    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            if fn() != engine.TN_OK:
                raise RuntimeError(lib.tn_last_error().decode())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round

    est = sample(launches[pilot], 3)
    rounds = max(5, min(500, int(20.0 / est)))    # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for fn in launches.values():
            sample(fn, rounds)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds))
    ms = {}
    for key, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        ms[key] = {"median": med, "min": s[0], "max": s[-1], "spread": (s[-1] - s[0]) / med}
    return rounds, ms


def run_point(point, tag, size, repeats):
    sys.path.insert(0, ROOT)
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, out_rows, vectors = SHAPES[tag]
    plan = engine.Plan(n, q, psi)
    # (the C entry points directly: at cfg3 a launch is short enough for the Python wrappers' checks to show)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    row = n * plan.elem_bytes
    ok = engine.TN_OK
    extra = {}

    def empty(rows):
        return torch.empty((rows, n), dtype=plan.torch_dtype, device=f"cuda:{plan.device}")

    if point == "matvec":
        k = l = size
        mat = plan.prepare(plan.fill_lcg(k * l, 11, 2)).tensor                # A[i][j] at row i * l + j
        s = plan.fill_lcg(vectors * l, 12, 2)                                  # s[v][j] at row v * l + j
        shat, c_new, c_base = empty(vectors * l), empty(k * vectors), empty(k * vectors)
        ps, pm, psh, pn, pb = (t.data_ptr() for t in (s, mat, shat, c_new, c_base))
        block = vectors * row

        def new():
            st_ = lib.tn_prepare_dev(h, ps, psh, vectors * l, st)
            for i in range(k):
                st_ |= lib.tn_poly_dot_hat_dev(h, psh, pm + i * l * row, 1, pn + i * block, vectors, l, 0, st)
            return st_

        def base():
            st_ = ok
            for i in range(k):
                st_ |= lib.tn_poly_dot_prepared_dev(h, ps, pm + i * l * row, 1, pb + i * block, vectors, l, st)
            return st_

        launches, pilot, batch = {"new": new, "base": base}, "base", vectors
        for fn in launches.values():
            assert fn() == ok, lib.tn_last_error().decode()
        torch.cuda.synchronize()
        identical = bool(torch.equal(c_new, c_base))
        extra = {"transforms": {"new": l + k, "base": k * (l + 1)}}
    elif point == "term":
        terms, batch = size, out_rows
        rows = batch * terms
        a = plan.fill_lcg(rows, 1, 2)
        ahat = plan.prepare(a).tensor
        bhat = plan.prepare(plan.fill_lcg(rows, 2, 2)).tensor
        outs = {key: empty(batch) for key in ("hat_shared", "hat_per_set", "kept_shared", "kept_per_set", "dot_shared", "dot_per_set")}
        pa, pah, pbh = a.data_ptr(), ahat.data_ptr(), bhat.data_ptr()
        po = {key: t.data_ptr() for key, t in outs.items()}
        launches = {
            "hat_shared": lambda: lib.tn_poly_dot_hat_dev(h, pah, pbh, 1, po["hat_shared"], batch, terms, 0, st),
            "hat_per_set": lambda: lib.tn_poly_dot_hat_dev(h, pah, pbh, batch, po["hat_per_set"], batch, terms, 0, st),
            "kept_shared": lambda: lib.tn_poly_dot_hat_dev(h, pah, pbh, 1, po["kept_shared"], batch, terms, 1, st),
            "kept_per_set": lambda: lib.tn_poly_dot_hat_dev(h, pah, pbh, batch, po["kept_per_set"], batch, terms, 1, st),
            "dot_shared": lambda: lib.tn_poly_dot_prepared_dev(h, pa, pbh, 1, po["dot_shared"], batch, terms, st),
            "dot_per_set": lambda: lib.tn_poly_dot_prepared_dev(h, pa, pbh, batch, po["dot_per_set"], batch, terms, st),
        }
        pilot = "dot_per_set"
        for fn in launches.values():
            assert fn() == ok, lib.tn_last_error().decode()
        torch.cuda.synchronize()
        identical = True
        for mode in ("shared", "per_set"):
            identical = identical and bool(torch.equal(outs["hat_" + mode], outs["dot_" + mode]))
            back = plan.unprepare(engine.PreparedOperand(plan, outs["kept_" + mode], batch))
            identical = identical and bool(torch.equal(back, outs["dot_" + mode]))
        # rows a launch reads and writes, per output row
        extra = {"rows_moved": {"hat_shared": terms + 1, "hat_per_set": 2 * terms + 1, "kept_shared": terms + 1, "kept_per_set": 2 * terms + 1,
                                "dot_shared": terms + 1, "dot_per_set": 2 * terms + 1}}
        copy_dst = empty(batch)

        def copy():
            copy_dst.copy_(outs["dot_shared"])
            return ok
        launches["d2d_copy"] = copy
        extra["rows_moved"]["d2d_copy"] = 2
    else:
        batch = out_rows
        x = plan.fill_lcg(batch, 1, 2)
        xhat, back, y, z = empty(batch), empty(batch), empty(batch), empty(batch)
        px, pxh, pb_, py, pz = (t.data_ptr() for t in (x, xhat, back, y, z))
        launches = {
            "unprepare": lambda: lib.tn_unprepare_dev(h, pxh, pb_, batch, st),
            "prepare": lambda: lib.tn_prepare_dev(h, px, py, batch, st),
            "ntt_inverse": lambda: lib.tn_ntt_inverse_dev(h, px, pz, batch, engine.VARIANTS["fused"], st),
        }
        pilot = "prepare"
        assert lib.tn_prepare_dev(h, px, pxh, batch, st) == ok, lib.tn_last_error().decode()
        for fn in launches.values():
            assert fn() == ok, lib.tn_last_error().decode()
        torch.cuda.synchronize()
        identical = bool(torch.equal(back, x)) and bool(torch.equal(y, xhat))          # fill_lcg words are canonical
        extra = {"rows_moved": {key: 2 for key in launches}}

    rounds, ms = measure(torch, engine, lib, launches, repeats, pilot)
    out = {"point": point, "shape": name, "size": size, "batch": batch, "rounds_per_sample": rounds, "repeats": repeats, "identical": identical,
           "row_bytes": row, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": ms}
    out.update(extra)
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def report(results, resources):
    lines = ["Transform-domain products: tn_poly_dot_hat_dev / tn_unprepare_dev against the parent's best way to the same bits (tools/gpu_hat.py)", ""]
    for r in results:
        what = {"matvec": f"matrix-vector k = l = {r['size']}, {r['batch']} vectors", "term": f"per-term cost, terms {r['size']}, {r['batch']} output rows",
                "unprep": f"unprepare, {r['batch']} rows"}[r["point"]]
        lines.append(f"{r['shape']}, {what}   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; outputs identical: {r['identical']}")
        if "transforms" in r:
            lines.append(f"  transforms per vector: new {r['transforms']['new']}, base {r['transforms']['base']}")
        for key, m in r["ms"].items():
            rate = ""
            if "rows_moved" in r:
                rate = f"   {r['rows_moved'][key] * r['batch'] * r['row_bytes'] / (m['median'] * 1e-3) / 1e12:6.3f} TB/s"
            lines.append(f"  {key:13s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %{rate}")
        for new, base in PAIRS[r["point"]]:
            d, m = r["ms"][new], r["ms"][base]
            verdict = "faster, ranges disjoint" if d["max"] < m["min"] else "NOT faster by disjoint ranges"
            lines.append(f"  {new} / {base}: x{d['median'] / m['median']:6.3f}   {verdict}")
        lines.append("")
    if resources:
        with open(resources) as f:
            lines.append(f.read().rstrip())
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--point", choices=sorted(PAIRS))
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cfg2")
    ap.add_argument("--size", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hat_domain_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.point:
        return run_point(args.point, args.shape, args.size, args.repeats)
    results = []
    for tag in ("cfg2", "cfg3"):
        for point, size in POINTS:
            step = f"{tag} {point} {size}"
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--point", point, "--shape", tag, "--size", str(size), "--repeats", str(args.repeats)],
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
