#!/usr/bin/env python3
"""Same-process A/B of the blind rotation from one launch (tn_poly_blind_rotate_prepared_dev) against the loop a caller has without it.

  gpu_blindrot.py [--out FILE] [--resources FILE] [--repeats N]            driver: one child process per point, each under its own
                                                                           time limit; nothing runs after a step that failed
  gpu_blindrot.py --shape S --terms T --batch B [--repeats N]              one point in this process; one JSON line

Shapes: n1024 = n 1024 / 24-bit, 64 steps (base_log 12, 8 for terms 2, 3); n2048 = n 2048 / 60-bit and n4096 = n 4096 / 60-bit,
16 steps (base_log 30, 20).  Batches 256 and 4,096.  Balanced digits, random exponents (any 32-bit word), one shared key per step.
In one process, after >= 0.15 s of warm launches,
  one_launch   tn_poly_blind_rotate_prepared_dev on acc = [batch][2][n]                                          one launch
  loop         `steps` direct calls of tn_poly_cmux_rotate_prepared_dev (bhat_sets = 1) over two alternating buffers on the same
               keys and exponents: the only route without the new call                                           steps launches
  loop_graph   the same `steps` launches replayed from one captured graph                                        one replay
are timed interleaved `repeats` times, K rounds per sample between two events recorded on the stream the kernels run on; the
output of the one launch is compared in full with the loop's (and the graph's) before anything is timed.  A point counts as
faster only where the new call's slowest repeat is below the other's fastest.
--resources appends a file (the resource table, taken where the library was built)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q60, PSI4096 = 1152921504606830593, 431606828070683274
SHAPES = {
    "n1024": ("n=1024 24-bit", 1024, 8380417, 5548360, 64, {2: 12, 3: 8}),
    "n2048": ("n=2048 60-bit", 2048, Q60, pow(PSI4096, 2, Q60), 16, {2: 30, 3: 20}),
    "n4096": ("n=4096 60-bit", 4096, Q60, PSI4096, 16, {2: 30, 3: 20}),
}
TERMS = (2, 3)
BATCHES = (256, 4096)
STEP_TIMEOUT_S = 120
KEYS = ("one_launch", "loop", "loop_graph")


def run_point(tag, terms, batch, repeats):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from tiny_ntt_amd import engine
    name, n, q, psi, steps, logs = SHAPES[tag]
    w, flags = logs[terms], engine.GADGET_BALANCED
    plan = engine.Plan(n, q, psi)
    key_rows = 4 * terms
    row_bytes = n * plan.elem_bytes
    acc = plan.fill_lcg(batch * 2, 1, 2).reshape(batch, 2, n)
    exps = torch.from_numpy(np.random.default_rng(17).integers(0, 2 ** 32, (steps, batch), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(acc.device)
    bhat = plan.prepare(plan.fill_lcg(steps * key_rows, 2, 2)).tensor                            # [steps][2][2][terms][n]
    c, c_graph = torch.empty_like(acc), torch.empty_like(acc)
    bufs, gbufs = [torch.empty_like(acc), torch.empty_like(acc)], [torch.empty_like(acc), torch.empty_like(acc)]
    lib, h = plan._lib, plan._h
    P = lambda t: t.data_ptr()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        st = plan._stream_ptr(None)                    # torch's current stream: `side`

        def one_launch():
            return lib.tn_poly_blind_rotate_prepared_dev(h, P(acc), P(exps), P(bhat), P(c), batch, 2, steps, terms, w, flags, st)

        def loop_into(two):
            src, rc = acc, 0
            for k in range(steps):
                dst = two[k & 1]
                rc |= lib.tn_poly_cmux_rotate_prepared_dev(h, P(src), P(exps) + 4 * k * batch, P(bhat) + k * key_rows * row_bytes, 1, P(dst), batch, 2, terms, w,
                                                           flags, st)
                src = dst
            return rc

        assert one_launch() == engine.TN_OK, lib.tn_last_error().decode()
        assert loop_into(bufs) == engine.TN_OK, lib.tn_last_error().decode()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assert loop_into(gbufs) == engine.TN_OK
        graph.replay()
        side.synchronize()
        last = (steps - 1) & 1
        identical = bool(torch.equal(c, bufs[last])) and bool(torch.equal(c, gbufs[last]))

        def replay():
            graph.replay()
            return engine.TN_OK

        launches = {"one_launch": one_launch, "loop": lambda: loop_into(bufs), "loop_graph": replay}

        def sample(fn, rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                if fn() != engine.TN_OK:
                    raise RuntimeError(lib.tn_last_error().decode())
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / rounds       # ms per round (one blind rotation, by whichever route)

        est = sample(launches["loop"], 3)
        rounds = max(3, min(200, int(20.0 / est)))    # ~20 ms of launches per sample
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:        # the shader clock settles ~0.1 s after idle
            for fn in launches.values():
                sample(fn, rounds)
        times = {key: [] for key in launches}
        for _ in range(repeats):
            for key, fn in launches.items():
                times[key].append(sample(fn, rounds))
    out = {"shape": name, "tag": tag, "batch": batch, "steps": steps, "terms": terms, "base_log": w, "rounds_per_sample": rounds, "repeats": repeats,
           "identical": identical, "build_id": engine.build_id(), "device": torch.cuda.get_device_name(0), "ms": {}}
    for key, v in times.items():
        srt = sorted(v)
        med = srt[len(srt) // 2]
        out["ms"][key] = {"median": med, "min": srt[0], "max": srt[-1], "spread": (srt[-1] - srt[0]) / med}
    del graph
    plan.close()
    print(json.dumps(out), flush=True)
    return 0 if identical else 1


def line(key, m):
    return f"  {key:12s} median {m['median'] * 1e3:10.2f} us   min {m['min'] * 1e3:10.2f}   max {m['max'] * 1e3:10.2f}   spread {100 * m['spread']:5.2f} %"


def verdict(g, base):
    if g["max"] < base["min"]:
        return "faster, ranges disjoint"
    if g["min"] > base["max"]:
        return "SLOWER, ranges disjoint"
    return "WITHIN THE SPREAD"


def report(results, resources):
    lines = ["Blind rotation: one tn_poly_blind_rotate_prepared_dev launch against `steps` tn_poly_cmux_rotate_prepared_dev launches over two "
             "alternating buffers on the same keys and exponents (loop), and against those launches replayed from one captured graph "
             "(loop_graph) (tools/gpu_blindrot.py)",
             "A point counts as faster only where the new call's slowest repeat is below the other's fastest.", ""]
    for r in results:
        lines.append(f"{r['shape']}, batch {r['batch']}, steps {r['steps']}, terms {r['terms']}, base_log {r['base_log']}, balanced digits, random exponents   "
                     f"build {r['build_id']}   {r['device']}")
        lines.append(f"  {r['repeats']} interleaved repeats of {r['rounds_per_sample']} rounds each; every word identical to the loop and to the graph: {r['identical']}")
        for key in KEYS:
            lines.append(line(key, r["ms"][key]))
        g, lp, gr = (r["ms"][key] for key in KEYS)
        lines.append(f"  one_launch: x{g['median'] / lp['median']:6.3f} of the loop ({verdict(g, lp)}); x{g['median'] / gr['median']:6.3f} of the graph "
                     f"({verdict(g, gr)}); per step {g['median'] * 1e3 / r['steps']:8.2f} us against {lp['median'] * 1e3 / r['steps']:8.2f} and "
                     f"{gr['median'] * 1e3 / r['steps']:8.2f}")
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
    ap.add_argument("--batch", type=int)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blindrot_ab.txt"))
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.shape:
        return run_point(args.shape, args.terms or 2, args.batch or 256, args.repeats)
    results = []
    for tag in ("n1024", "n2048", "n4096"):
        for terms in TERMS:
            for batch in BATCHES:
                rc, res = child(args, ["--shape", tag, "--terms", str(terms), "--batch", str(batch)], f"{tag} terms {terms} batch {batch}")
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
