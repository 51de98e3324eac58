#!/usr/bin/env python3
"""Same-process A/B of the automorphism calls against the routes a caller has without them.

  gpu_galois.py [--out FILE] [--repeats N] [--shape cfg2|cfg3]

Shapes: cfg2 = n 4096 / 60-bit / 65,536 rows, cfg3 = n 1024 / 24-bit / 4,096 rows (the points of tools/gpu_gadget2.py).
Elements g in {3, 5, 2n - 1, one seeded}.  In one process, after >= 0.15 s of warm launches, per shape:
  copy               a device-to-device copy of the same number of rows (the floor: 2 rows of traffic per row)
  coeff g            tn_automorphism_dev, count = 1                            (2 rows of traffic per row)
  coeff torch g      today's route on coefficients: index_select, q - x, where, on the plan's dtype (canonical inputs)
  coeff x4           tn_automorphism_dev, count = 4, the four elements         (5 rows of traffic per row)
  coeff 4x1          four count = 1 launches
  prep g             tn_automorphism_prepared_dev, count = 1
  prep route g       today's route on prepared rows: tn_unprepare_dev, the torch route, tn_prepare_dev
  prep x4, prep 4x1  as above
  key switch         one tn_poly_gadget_multidot_prepared_dev launch on the same rows (outs 2, terms 2, shared key): what a
                     rotation's automorphism stands beside
are timed interleaved `repeats` times, K rounds per sample between two events recorded on the stream the kernels run on.
Every output is compared for equality before timing.  A call counts as faster only where its slowest repeat is below the
route's fastest.  Achieved bytes per second: rows * (1 + count) * row bytes / median time."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "cfg2": ("n=4096 60-bit", 4096, 1152921504606830593, 431606828070683274, 65536, 30),
    "cfg3": ("n=1024 24-bit", 1024, 8380417, 5548360, 4096, 12),
}


def torch_route(torch, n, q, g, device):
    """The gather-negate-select a caller can write today: out[d] = a[src[d]], negated (0 stays 0) where the image wraps."""
    ginv = pow(g, -1, 2 * n)
    u = [d * ginv % (2 * n) for d in range(n)]
    src = torch.tensor([v % n for v in u], dtype=torch.int64, device=device)
    neg = torch.tensor([v >= n for v in u], dtype=torch.bool, device=device)

    def run(a):
        v = a.index_select(1, src)
        w = torch.where(v != 0, q - v, v)
        return torch.where(neg, w, v)
    return run


def run_shape(tag, repeats):
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, batch, w = SHAPES[tag]
    plan = engine.Plan(n, q, psi)
    lib, h, st = plan._lib, plan._h, plan._stream_ptr(None)
    dev = f"cuda:{plan.device}"
    elements = [3, 5, 2 * n - 1, (2 * 0x9E3779B1 % (2 * n)) | 1]
    a = plan.fill_lcg(batch, 1, 2)                                              # canonical residues
    ahat = plan.prepare(a).tensor
    out1 = torch.empty_like(a); out1b = torch.empty_like(a)
    out4 = torch.empty((batch, 4, n), dtype=a.dtype, device=dev); out4b = torch.empty((4, batch, n), dtype=a.dtype, device=dev)
    tmp = torch.empty_like(a)
    ksk = plan.prepare(plan.fill_lcg(4, 9, 2)).tensor                          # a shared key: outs 2 x terms 2 rows
    ks = torch.empty((batch, 2, n), dtype=a.dtype, device=dev)
    garr = {g: (ctypes.c_uint32 * 1)(g) for g in elements}
    gall = (ctypes.c_uint32 * 4)(*elements)
    routes = {g: torch_route(torch, n, q, g, dev) for g in elements}
    ok = engine.TN_OK

    def must(status):
        if status != ok:
            raise RuntimeError(lib.tn_last_error().decode())

    def prep_route(g, dst):
        must(lib.tn_unprepare_dev(h, ahat.data_ptr(), tmp.data_ptr(), batch, st))
        r = routes[g](tmp)
        must(lib.tn_prepare_dev(h, r.data_ptr(), dst.data_ptr(), batch, st))

    launches = {"copy": lambda: out1.copy_(a)}
    for g in elements:
        launches[f"coeff g={g}"] = lambda g=g: must(lib.tn_automorphism_dev(h, a.data_ptr(), out1.data_ptr(), batch, garr[g], 1, st))
        launches[f"coeff torch g={g}"] = lambda g=g: routes[g](a)
        launches[f"prep g={g}"] = lambda g=g: must(lib.tn_automorphism_prepared_dev(h, ahat.data_ptr(), out1.data_ptr(), batch, garr[g], 1, st))
        launches[f"prep route g={g}"] = lambda g=g: prep_route(g, out1b)
    launches["coeff x4"] = lambda: must(lib.tn_automorphism_dev(h, a.data_ptr(), out4.data_ptr(), batch, gall, 4, st))
    launches["coeff 4x1"] = lambda: [must(lib.tn_automorphism_dev(h, a.data_ptr(), out4b[m].data_ptr(), batch, garr[g], 1, st)) for m, g in enumerate(elements)]
    launches["prep x4"] = lambda: must(lib.tn_automorphism_prepared_dev(h, ahat.data_ptr(), out4.data_ptr(), batch, gall, 4, st))
    launches["prep 4x1"] = lambda: [must(lib.tn_automorphism_prepared_dev(h, ahat.data_ptr(), out4b[m].data_ptr(), batch, garr[g], 1, st))
                                    for m, g in enumerate(elements)]
    launches["key switch"] = lambda: must(lib.tn_poly_gadget_multidot_prepared_dev(h, a.data_ptr(), ksk.data_ptr(), 1, ks.data_ptr(), batch, 2, 2, w,
                                                                               engine.GADGET_BALANCED, st))

    # equality before timing: the new calls against the routes, the four-element calls against the single ones
    identical = True
    for g in elements:
        launches[f"coeff g={g}"]()
        identical &= bool(torch.equal(out1, routes[g](a)))
        launches[f"prep g={g}"]()
        prep_route(g, out1b)
        identical &= bool(torch.equal(out1, out1b))
    for fam in ("coeff", "prep"):
        launches[f"{fam} x4"](); launches[f"{fam} 4x1"]()
        identical &= all(bool(torch.equal(out4[:, m], out4b[m])) for m in range(4))
    torch.cuda.synchronize()

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round

    rounds = {key: max(3, min(500, int(20.0 / max(sample(fn, 3), 1e-3)))) for key, fn in launches.items()}     # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for key, fn in launches.items():
            sample(fn, 3)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds[key]))
    res = {"shape": name, "tag": tag, "batch": batch, "n": n, "row_bytes": n * plan.elem_bytes, "elements": elements, "repeats": repeats,
           "identical": identical, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        res["ms"][key] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": rounds[key]}
    plan.close()
    print(json.dumps(res), flush=True)
    return res


def rows_moved(key):
    return 5 if key.endswith("x4") else 8 if key.endswith("4x1") else 2


def report(results):
    lines = ["Ring automorphisms: tn_automorphism_dev and tn_automorphism_prepared_dev against a device-to-device copy and against the routes a "
             "caller has without them (tools/gpu_galois.py)", ""]
    for r in results:
        lines.append(f"{r['shape']}, {r['batch']} rows, elements {r['elements']}   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats; every output identical to its route's / to the single-element calls: {r['identical']}")
        for key, m in r["ms"].items():
            tb = ""
            if not key.startswith("key") and "route" not in key and "torch" not in key:
                tb = f"   {r['batch'] * rows_moved(key) * r['row_bytes'] / (m['median'] * 1e-3) / 1e12:5.2f} TB/s"
            lines.append(f"  {key:22s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   ({m['rounds']} rounds){tb}")
        pairs = [(f"coeff g={g}", f"coeff torch g={g}") for g in r["elements"]] + [(f"prep g={g}", f"prep route g={g}") for g in r["elements"]]
        pairs += [("coeff x4", "coeff 4x1"), ("prep x4", "prep 4x1")]
        for new, old in pairs:
            a, b = r["ms"][new], r["ms"][old]
            verdict = "faster, ranges disjoint" if a["max"] < b["min"] else ("SLOWER, ranges disjoint" if a["min"] > b["max"] else "NOT faster by disjoint ranges")
            lines.append(f"  {new} / {old}: x{a['median'] / b['median']:6.3f}   {verdict}")
        c = r["ms"]["copy"]["median"]
        for key in [f"coeff g={r['elements'][1]}", f"prep g={r['elements'][1]}", "coeff x4", "prep x4"]:
            lines.append(f"  {key} / copy: x{r['ms'][key]['median'] / c:6.3f} in time for x{rows_moved(key) / 2:4.2f} the traffic")
        lines.append(f"  coeff g={r['elements'][1]} / key switch (outs 2, terms 2, shared key): x{r['ms']['coeff g=%d' % r['elements'][1]]['median'] / r['ms']['key switch']['median']:6.3f}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES), help="one shape only (default: both)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "galois_ab.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    results = [run_shape(tag, args.repeats) for tag in ([args.shape] if args.shape else ["cfg2", "cfg3"])]
    text = report(results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
