#!/usr/bin/env python3
"""Timing of the LWE calls (tn_lwe_modswitch_dev, tn_sample_extract_dev, tn_lwe_keyswitch_dev) and their share of Plan.bootstrap.

  gpu_lwe.py [--out FILE] [--repeats N] [--point TAG]

Points: n = 1024 / 24-bit with n_out = 512, key-switch (terms, w) = (3, 8) and (6, 4); n = 2048 / 60-bit with n_out = 768, (4, 15);
each at batch 256 and 4,096.  One process per point (the parent never opens the GPU).  Per point, after the outputs are compared
and >= 0.15 s of warm launches, these are timed interleaved `repeats` times, K rounds per sample between two events:
  modswitch          tn_lwe_modswitch_dev on [batch][n_out + 1] (the rows a bootstrap switches: dim = n_out)
  copy (modswitch)   a device-to-device copy that moves the same bytes (half of input + output each way)
  extract            tn_sample_extract_dev on [batch][2][n], index 0
  copy (extract)     a device-to-device copy of batch * n words (the call reads the c1 rows and writes n + 1 words per row)
  keyswitch          tn_lwe_keyswitch_dev [batch][n + 1] -> [batch][n_out + 1], unsigned digits
  float64 route      24-bit only, what a caller has today: digits from torch shifts and masks, a float64 torch.matmul (exact: the
                     sums stay below 2^53), the body added, % q.  There is NO such route at 60-bit: torch has no 128-bit sum.
  bootstrap          Plan.bootstrap on the same rows: dim = n_out steps, bootstrap key balanced (3, 8) / (3, 20), one launch at batch
                     256 and the step loop at 4,096 (the README's guidance), random keys (timing only)
Outputs compared first: modswitch and keyswitch in full against torch int64 / float64 at 24-bit; at 60-bit the first and last row
of each against Python integers (no device route exists); the extraction in full against torch (flip, q - x) at both.  A call
counts as faster only where its slowest repeat is below the other's fastest."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q60, PSI4096 = 1152921504606830593, 431606828070683274
SHAPES = {
    "n1024": ("n=1024 24-bit", 1024, 8380417, 5548360, 512, (3, 8)),
    "n2048": ("n=2048 60-bit", 2048, Q60, pow(PSI4096, 2, Q60), 768, (3, 20)),
}
POINTS = [("n1024", b, p) for b in (256, 4096) for p in ((3, 8), (6, 4))] + [("n2048", b, (4, 15)) for b in (256, 4096)]


def point_tag(p):
    return f"{p[0]}-b{p[1]}-t{p[2][0]}w{p[2][1]}"


def run_point(tag, batch, pair, repeats):
    import numpy as np
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, n_out, (bt, bw) = SHAPES[tag]
    terms, w = pair
    plan = engine.Plan(n, q, psi)
    dev = f"cuda:{plan.device}"
    td = plan.torch_dtype
    g = torch.Generator(device=dev); g.manual_seed(5)
    rnd = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=g).to(td)       # canonical words
    small, acc, big = rnd(batch, n_out + 1), rnd(batch, 2, n), rnd(batch, n + 1)
    ksk = rnd(n, terms, n_out + 1)
    bsk = plan.prepare(plan.fill_lcg(n_out * 4 * bt, 3, 2))
    tv = rnd(1, n)
    exps = torch.empty((n_out + 1, batch), dtype=torch.int32, device=dev)
    ext = torch.empty((batch, n + 1), dtype=td, device=dev)
    out = torch.empty((batch, n_out + 1), dtype=td, device=dev)
    ms_bytes = (small.numel() * plan.elem_bytes + exps.numel() * 4) // 2
    cp_a, cp_b = torch.empty(ms_bytes, dtype=torch.uint8, device=dev), torch.empty(ms_bytes, dtype=torch.uint8, device=dev)
    cx_a, cx_b = torch.empty((batch, n), dtype=td, device=dev), torch.empty((batch, n), dtype=td, device=dev)

    launches = {
        "modswitch": lambda: plan.lwe_modswitch(small, out=exps),
        "copy (modswitch)": lambda: cp_b.copy_(cp_a),
        "extract": lambda: plan.sample_extract(acc, 0, out=ext),
        "copy (extract)": lambda: cx_b.copy_(cx_a),
        "keyswitch": lambda: plan.lwe_keyswitch(big, ksk, n_out, terms, w, out=out),
        "bootstrap": lambda: plan.bootstrap(small, bsk, tv, ksk, terms=bt, base_log=bw, ks_terms=terms, ks_base_log=w, balanced=True,
                                            one_launch=batch <= 256),
    }
    f64 = None
    if q < 2 ** 31:
        kf = ksk.reshape(n * terms, n_out + 1).to(torch.float64)
        shifts = torch.arange(terms, device=dev, dtype=torch.int64) * w

        def f64():
            x = big[:, :n].to(torch.int64)
            d = ((x[:, :, None] >> shifts) & ((1 << w) - 1)).reshape(batch, n * terms).to(torch.float64)
            r = torch.matmul(d, kf)
            r[:, n_out] += big[:, n].to(torch.float64)
            return torch.remainder(r, float(q)).to(td)
        launches["float64 route"] = f64

    # ---- outputs first ----
    def ints(t):
        return [int(v) & (2 ** (8 * plan.elem_bytes) - 1) for v in t.cpu().reshape(-1).tolist()]

    identical = True
    launches["modswitch"](); launches["extract"](); launches["keyswitch"]()
    c1 = acc[:, 1].to(torch.int64)
    want = torch.cat([c1[:, :1], ((q - c1) % q).flip(1)[:, :n - 1], acc[:, 0, :1].to(torch.int64)], dim=1)
    identical &= bool(torch.equal(ext.to(torch.int64), want))
    if f64 is not None:
        identical &= bool(torch.equal(out, f64()))
        identical &= bool(torch.equal(exps.to(torch.int64), (((2 * n * small.to(torch.int64) + q // 2) // q) % (2 * n)).t()))
        compared = "in full against torch"
    else:
        kk = np.array(ints(ksk), dtype=object).reshape(n * terms, n_out + 1)
        for r in (0, batch - 1):
            row = ints(big[r])
            d = np.array([(x >> (j * w)) & ((1 << w) - 1) for x in row[:n] for j in range(terms)], dtype=object)
            ref = d.dot(kk)
            ref[n_out] += row[n]
            identical &= [int(v) % q for v in ref] == ints(out[r])
            identical &= [((2 * n * x + q // 2) // q) % (2 * n) for x in ints(small[r])] == [int(v) for v in exps[:, r].cpu().tolist()]
        compared = "rows 0 and batch - 1 against Python integers (modswitch, keyswitch); extraction in full against torch"
    torch.cuda.synchronize()

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round

    rounds = {key: max(1, min(500, int(20.0 / max(sample(fn, 2), 1e-3)))) for key, fn in launches.items()}     # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for key, fn in launches.items():
            if key != "bootstrap":
                sample(fn, 3)
    times = {key: [] for key in launches}
    for _ in range(repeats):
        for key, fn in launches.items():
            times[key].append(sample(fn, rounds[key]))
    res = {"shape": name, "tag": tag, "batch": batch, "n": n, "n_out": n_out, "terms": terms, "w": w, "repeats": repeats, "identical": identical,
           "compared": compared, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        s = sorted(v)
        res["ms"][key] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": rounds[key]}
    plan.close()
    print("RESULT " + json.dumps(res), flush=True)
    return 0 if identical else 1


def verdict(a, b):
    return "faster, ranges disjoint" if a["max"] < b["min"] else ("SLOWER, ranges disjoint" if a["min"] > b["max"] else "ranges overlap")


def report(results):
    lines = ["LWE ends of the bootstrap: tn_lwe_modswitch_dev, tn_sample_extract_dev and tn_lwe_keyswitch_dev against device-to-device copies, "
             "against the float64 route a caller has today (24-bit only) and inside Plan.bootstrap (tools/gpu_lwe.py)", ""]
    for r in results:
        lines.append(f"{r['shape']}, n_out {r['n_out']}, batch {r['batch']}, key switch terms {r['terms']} w {r['w']}   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats, one process; outputs identical: {r['identical']} ({r['compared']})")
        for key, m in r["ms"].items():
            lines.append(f"  {key:18s} median {m['median'] * 1e3:11.2f} us   min {m['min'] * 1e3:11.2f}   max {m['max'] * 1e3:11.2f}   ({m['rounds']} rounds)")
        ms = r["ms"]
        for call, copy in (("modswitch", "copy (modswitch)"), ("extract", "copy (extract)")):
            lines.append(f"  {call} / {copy}: x{ms[call]['median'] / ms[copy]['median']:6.3f}   {verdict(ms[call], ms[copy])}")
        if "float64 route" in ms:
            lines.append(f"  keyswitch / float64 route: x{ms['keyswitch']['median'] / ms['float64 route']['median']:6.3f}   {verdict(ms['keyswitch'], ms['float64 route'])}")
        else:
            lines.append("  keyswitch / float64 route: no such route at 60-bit (no 128-bit accumulate in torch)")
        macs = r["batch"] * r["n"] * r["terms"] * (r["n_out"] + 1)
        lines.append(f"  keyswitch: {macs / (ms['keyswitch']['median'] * 1e-3) / 1e12:6.3f} T multiply-adds / s")
        lines.append(f"  keyswitch / bootstrap: {100 * ms['keyswitch']['median'] / ms['bootstrap']['median']:5.2f} % of the whole bootstrap's time")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--point", help="one point only, e.g. n1024-b256-t3w8 (runs in this process)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lwe_ab.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.point:
        p = next(p for p in POINTS if point_tag(p) == args.point)
        return run_point(p[0], p[1], p[2], args.repeats)
    results, rc = [], 0
    for p in POINTS:                                  # one process per point, one after the other; stop at the first that fails
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--point", point_tag(p), "--repeats", str(args.repeats)],
                           stdout=subprocess.PIPE, text=True, timeout=600)
        sys.stdout.write(r.stdout)
        if r.returncode not in (0, 1):
            print(f"{point_tag(p)}: exit status {r.returncode}; nothing more is started", flush=True)
            return r.returncode
        rc |= r.returncode
        results += [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]
    text = report(results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
