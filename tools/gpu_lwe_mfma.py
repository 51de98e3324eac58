#!/usr/bin/env python3
"""Timing of the key switch from a prepared key on the matrix cores (tn_lwe_ksk_prepare_dev, tn_lwe_keyswitch_prepared_dev) against
tn_lwe_keyswitch_dev on the same buffers in the same process, against the float64 torch.matmul route of tools/gpu_lwe.py (24-bit
only) and inside Plan.bootstrap.

  gpu_lwe_mfma.py [--out FILE] [--repeats N] [--point TAG]

Points: the six of tools/gpu_lwe.py (n = 1024 / 24-bit with n_out = 512, key-switch (terms, w) = (3, 8) and (6, 4); n = 2048 /
60-bit with n_out = 768, (4, 15); each at batch 256 and 4,096), unsigned digits.  The prepared call takes digits of a signed byte
only, so next to the table's pair every point has its byte-wide pair: (6, 4) unsigned is its own; (3, 8) and (4, 15) are not, and
get their balanced twin at base_log 8, (3, 8) balanced and (8, 8) balanced (8 digits of 8 bits cover 60 bits; a key of twice the
rows).  One process per point (the parent never opens the GPU).  Per point, after the outputs are compared and >= 0.15 s of warm
launches, these are timed interleaved `repeats` times, K rounds per sample between two events:
  plain (table)      tn_lwe_keyswitch_dev at the table's pair, [batch][n + 1] -> [batch][n_out + 1]
  plain (byte)       tn_lwe_keyswitch_dev at the byte-wide pair (where it differs from the table's)
  prepared (byte)    tn_lwe_keyswitch_prepared_dev at the byte-wide pair, key prepared before
  float64 (table), float64 (byte)   24-bit only: digits cut in torch (unsigned, or balanced with the carry), a float64 torch.matmul,
                     the body added, % q.  No such route at 60-bit.
  prepare            tn_lwe_ksk_prepare_dev of the byte-wide key (its cost is paid once per key)
  bootstrap plain, bootstrap prepared   Plan.bootstrap on the same rows with the plain key at the table's pair and with the prepared
                     key at the byte-wide pair: dim = n_out steps, bootstrap key balanced (3, 8) / (3, 20), one launch at batch 256
                     and the step loop at 4,096, random keys (timing only)
Outputs compared first, in full: prepared (byte) against plain (byte) with torch.equal, and both against the float64 route at
24-bit.  A call counts as faster only where its slowest repeat is below the other's fastest.  The int8 rate counts L(q) byte
products per digit and key word and stands beside the machine's dense int8 peak, twice BF16's ~2.5 PFLOP/s: ~2.5 P multiply-adds/s."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q60, PSI4096 = 1152921504606830593, 431606828070683274
INT8_PEAK_MACS = 2.5e15
SHAPES = {
    "n1024": ("n=1024 24-bit", 1024, 8380417, 5548360, 512, (3, 8)),
    "n2048": ("n=2048 60-bit", 2048, Q60, pow(PSI4096, 2, Q60), 768, (3, 20)),
}
BYTE_PAIR = {(3, 8): (3, 8, True), (6, 4): (6, 4, False), (4, 15): (8, 8, True)}        # table's pair -> (terms, w, balanced)
POINTS = [("n1024", b, p) for b in (256, 4096) for p in ((3, 8), (6, 4))] + [("n2048", b, (4, 15)) for b in (256, 4096)]


def point_tag(p):
    return f"{p[0]}-b{p[1]}-t{p[2][0]}w{p[2][1]}"


def run_point(tag, batch, pair, repeats):
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, n_out, (bt, bw) = SHAPES[tag]
    terms, w = pair
    bterms, bw8, bbal = BYTE_PAIR[pair]
    same_pair = (bterms, bw8, bbal) == (terms, w, False)
    plan = engine.Plan(n, q, psi)
    dev = f"cuda:{plan.device}"
    td = plan.torch_dtype
    g = torch.Generator(device=dev); g.manual_seed(5)
    rnd = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=g).to(td)       # canonical words
    small, big = rnd(batch, n_out + 1), rnd(batch, n + 1)
    ksk_t = rnd(n, terms, n_out + 1)
    ksk_b = ksk_t if same_pair else rnd(n, bterms, n_out + 1)
    key = plan.lwe_ksk_prepare(ksk_b, bterms)
    scratch = torch.empty_like(key.tensor)
    bsk = plan.prepare(plan.fill_lcg(n_out * 4 * bt, 3, 2))
    tv = rnd(1, n)
    out_t, out_b, out_p = (torch.empty((batch, n_out + 1), dtype=td, device=dev) for _ in range(3))
    lib, stream = plan._lib, plan._stream_ptr(None)

    def prepare():
        st = lib.tn_lwe_ksk_prepare_dev(plan._h, ksk_b.data_ptr(), scratch.data_ptr(), n, n_out, bterms, stream)
        assert st == 0

    def boot(k, t_, w_, bal):
        return plan.bootstrap(small, bsk, tv, k, terms=bt, base_log=bw, ks_terms=t_, ks_base_log=w_, balanced=True, ks_balanced=bal,
                              one_launch=batch <= 256)
    launches = {"plain (table)": lambda: plan.lwe_keyswitch(big, ksk_t, n_out, terms, w, out=out_t)}
    if not same_pair:
        launches["plain (byte)"] = lambda: plan.lwe_keyswitch(big, ksk_b, n_out, bterms, bw8, bbal, out=out_b)
    launches["prepared (byte)"] = lambda: plan.lwe_keyswitch_prepared(big, key, bw8, bbal, out=out_p)
    launches["prepare"] = prepare
    launches["bootstrap plain"] = lambda: boot(ksk_t, terms, w, False)
    launches["bootstrap prepared"] = lambda: boot(key, bterms, bw8, bbal)

    def f64_route(ksk, t_, w_, bal):
        kf = ksk.reshape(n * t_, n_out + 1).to(torch.float64)
        B = 1 << w_

        shifts = torch.arange(t_, device=dev, dtype=torch.int64) * w_

        def run_unsigned():                        # tools/gpu_lwe.py's route, as it stands there
            x = big[:, :n].to(torch.int64)
            d = ((x[:, :, None] >> shifts) & (B - 1)).reshape(batch, n * t_).to(torch.float64)
            r = torch.matmul(d, kf)
            r[:, n_out] += big[:, n].to(torch.float64)
            return torch.remainder(r, float(q)).to(td)

        def run():                                 # balanced digits: the carry runs up the digits
            x = big[:, :n].to(torch.int64)
            carry, ds = torch.zeros_like(x), []
            for j in range(t_):
                d = ((x >> (j * w_)) & (B - 1)) + carry
                if bal:
                    carry = (d >= B // 2).to(torch.int64)
                    d = d - carry * B
                ds.append(d)
            r = torch.matmul(torch.stack(ds, dim=2).reshape(batch, n * t_).to(torch.float64), kf)
            r[:, n_out] += big[:, n].to(torch.float64)
            return torch.remainder(r, float(q)).to(td)
        return run if bal else run_unsigned
    if q < 2 ** 31:
        launches["float64 (table)"] = f64_route(ksk_t, terms, w, False)
        if not same_pair:
            launches["float64 (byte)"] = f64_route(ksk_b, bterms, bw8, bbal)

    # ---- outputs first ----
    identical = True
    for k_ in ("plain (table)", "plain (byte)", "prepared (byte)"):
        if k_ in launches:
            launches[k_]()
    identical &= bool(torch.equal(out_p, out_t if same_pair else out_b))
    compared = "prepared against plain at the byte-wide pair, in full"
    if q < 2 ** 31:
        identical &= bool(torch.equal(out_t, launches["float64 (table)"]()))
        identical &= bool(torch.equal(out_p, launches["float64 (table)" if same_pair else "float64 (byte)"]()))
        compared += "; both against the float64 route, in full"
    identical &= bool(torch.equal(boot(ksk_b, bterms, bw8, bbal), boot(key, bterms, bw8, bbal)))
    compared += "; Plan.bootstrap with the prepared key against the plain key at the byte-wide pair"
    torch.cuda.synchronize()

    def sample(fn, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rounds       # ms per round

    rounds = {k_: max(1, min(500, int(20.0 / max(sample(fn, 2), 1e-3)))) for k_, fn in launches.items()}     # ~20 ms of launches per sample
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
        for k_, fn in launches.items():
            if not k_.startswith("bootstrap"):
                sample(fn, 3)
    times = {k_: [] for k_ in launches}
    for _ in range(repeats):
        for k_, fn in launches.items():
            times[k_].append(sample(fn, rounds[k_]))
    res = {"shape": name, "tag": tag, "batch": batch, "n": n, "n_out": n_out, "pair": [terms, w], "byte_pair": [bterms, bw8, bbal], "repeats": repeats,
           "identical": identical, "compared": compared, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0),
           "limbs": key.tensor.numel() // (-(-(n_out + 1) // 16) * -(-(n * bterms) // 64) * 1024),
           "key_bytes": {"prepared": key.tensor.numel(), "plain (byte)": ksk_b.numel() * plan.elem_bytes, "plain (table)": ksk_t.numel() * plan.elem_bytes},
           "tiles": -(-batch // 64) * -(-(n_out + 1) // 64), "ms": {}}
    for k_, v in times.items():
        s = sorted(v)
        res["ms"][k_] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": rounds[k_]}
    plan.close()
    print("RESULT " + json.dumps(res), flush=True)
    return 0 if identical else 1


def verdict(a, b):
    return "faster, ranges disjoint" if a["max"] < b["min"] else ("SLOWER, ranges disjoint" if a["min"] > b["max"] else "ranges overlap")


def report(results):
    lines = ["LWE key switch from a prepared key on the matrix cores (tn_lwe_keyswitch_prepared_dev) against tn_lwe_keyswitch_dev and the float64 "
             "torch.matmul route on the same buffers, and inside Plan.bootstrap (tools/gpu_lwe_mfma.py)", ""]
    for r in results:
        bt, bw, bbal = r["byte_pair"]
        lines.append(f"{r['shape']}, n_out {r['n_out']}, batch {r['batch']}, table pair terms {r['pair'][0]} w {r['pair'][1]} unsigned, byte-wide pair terms {bt} "
                     f"w {bw} {'balanced' if bbal else 'unsigned'}   build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats, one process; outputs identical: {r['identical']} ({r['compared']})")
        ms = r["ms"]
        for k_, m in ms.items():
            lines.append(f"  {k_:20s} median {m['median'] * 1e3:11.2f} us   min {m['min'] * 1e3:11.2f}   max {m['max'] * 1e3:11.2f}   ({m['rounds']} rounds)")
        p = ms["prepared (byte)"]
        for other in ("plain (byte)", "plain (table)", "float64 (byte)", "float64 (table)"):
            if other in ms:
                lines.append(f"  prepared (byte) / {other}: x{p['median'] / ms[other]['median']:6.3f}   {verdict(p, ms[other])}")
        macs = r["batch"] * r["n"] * bt * (r["n_out"] + 1)
        rate = macs * r["limbs"] / (p["median"] * 1e-3)
        lines.append(f"  prepared (byte): {macs / (p['median'] * 1e-3) / 1e12:6.3f} T digit-by-word multiply-adds / s; {r['limbs']} limbs: {rate / 1e12:7.3f} T int8 "
                     f"multiply-adds / s, {100 * rate / INT8_PEAK_MACS:5.2f} % of the int8 peak (~2.5 P / s); {r['tiles']} tiles of 64 x 64 on the CUs")
        kb = r["key_bytes"]
        lines.append(f"  key bytes: prepared {kb['prepared']:,}; plain at the byte-wide pair {kb['plain (byte)']:,}; plain at the table's pair {kb['plain (table)']:,}; "
                     f"prepare pays for itself after {ms['prepare']['median'] / max(ms['plain (table)']['median'] - p['median'], 1e-9):5.2f} key switches against plain (table)")
        lines.append(f"  key switch / bootstrap: plain (table) {100 * ms['plain (table)']['median'] / ms['bootstrap plain']['median']:5.2f} % of bootstrap plain; "
                     f"prepared (byte) {100 * p['median'] / ms['bootstrap prepared']['median']:5.2f} % of bootstrap prepared; "
                     f"bootstrap prepared / bootstrap plain: x{ms['bootstrap prepared']['median'] / ms['bootstrap plain']['median']:6.3f}   "
                     f"{verdict(ms['bootstrap prepared'], ms['bootstrap plain'])}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--point", help="one point only, e.g. n1024-b256-t3w8 (runs in this process)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lwe_mfma_ab.txt"))
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
