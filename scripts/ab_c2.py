"""Same-box A/B of several builds of libmetran_hip.so on the NARROW full-output path, the headline of bench.py (configs[1]:
4096 x (8,2), T = 1000, no missing values, ``filter_smooth`` into preallocated buffers as bench.py's ``Workload`` does): every
library in its own child process (METRAN_HIP_LIBRARY), interleaved over ROUNDS rounds (at least three), ten warm-up launches
(the clock ramp, ``scripts/probe.py kernels --ramp``), kernel ms from hipEvents, the summed -2 log L and a checksum of every output array so
that a build that computes something else shows.  Name a library twice for the A/A spread.

  python scripts/ab_c2.py ab/parent.so ab/parent.so ab/new.so ab/new.so@general [--rounds 3] [--steps 20] [--B 8192] [--T 1000]
                          [--packed-sym] [--records filtered] [--missing 0.05]

``lib.so@general``: the same library with the record smoother's general covariance products at every step
(``set_variant("smoother16", "record_general")``: no rank-K step) -- a route of its own in the table.
``--missing F``: that fraction of the cells missing, so that wavefronts mix full and partly observed steps.

``--records filtered``: the filtered-record-only route (filter_kernel OUT = 3: ``simulate_smoothed`` on the records path).
Unlike ab_libs.py this stops at the FIRST child that does not exit with 0 and starts nothing more on the GPU after it."""
import json
import os
import subprocess
import sys

CHILD = r'''
import json, sys, torch
sys.path.insert(0, ".")
from metran_amd.engine import BatchedKalman
from metran_amd.synthetic import make_dfm_batch_torch
B, T, sym, filtered, steps = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3] == "1", sys.argv[4] == "1", int(sys.argv[5])
missing, route = float(sys.argv[6]), sys.argv[7]
dev = torch.device("cuda", 0)
d = make_dfm_batch_torch(B, 8, 2, T, seed=2000, device=dev, missing=missing)
kf = BatchedKalman(0, layout="time_major", packed_sym=sym)
if route == "general":
    kf.set_variant("smoother16", "record_general")
kf.projection_path = "records"
kf.set_observations(d["obs"]).set_loadings(d["loadings"])
if filtered:
    bufs = kf.alloc_projection(B)
    run = lambda: kf.simulate_smoothed(d["phi"], d["q"], buffers=bufs)
else:
    bufs = kf._alloc_outputs(B, ["F", "Pf", "Xp", "Pp", "S", "Ps"])
    run = lambda: kf.filter_smooth(d["phi"], d["q"], buffers=bufs)
for _ in range(10):
    run()
torch.cuda.synchronize()
kf.enable_timing(True, accumulate=True)
for _ in range(steps):
    run()
torch.cuda.synchronize()
f, fn, s, sn = kf.kernel_ms_totals()
chk = {}
for k in sorted(bufs):   # on the device, bit-exact: the int64 images summed plain and with position weights (wrapping integer sums)
    v = bufs[k]
    if not isinstance(v, torch.Tensor) or (not k.startswith("_rec") and v.dim() > 2 and "_rs" in bufs and k in ("F", "Pf", "Xp", "Pp", "S", "Ps")):
        continue         # (the views of a record array are covered by the array itself, pads included)
    bits = v.contiguous().view(-1).view(torch.int32 if v.element_size() == 4 else torch.int64).to(torch.int64)
    w = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 1021 + 1
    chk[k] = "%016x%016x" % (int(bits.sum()) & (2 ** 64 - 1), int((bits * w).sum()) & (2 ** 64 - 1))
print(json.dumps({"filter_ms": f / fn, "smoother_ms": s / sn, "mle_sum": float(kf.sum(bufs["mle"])), "chk": chk}))
'''


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    libs = [a for a in sys.argv[1:] if a.endswith((".so", ".so@general"))]
    rounds, steps, B, T = max(3, opt("--rounds", 3)), opt("--steps", 20), opt("--B", 4096), opt("--T", 1000)
    sym, filtered, missing = "--packed-sym" in sys.argv, opt("--records", "both") == "filtered", opt("--missing", 0.0)
    print("ab_c2: B = %d, T = %d, %s records, %s, %g of the cells missing, %d rounds of %d timed launches after 10 warm-up launches"
          % (B, T, "packed-symmetric" if sym else "full-square", "filtered record only" if filtered else "all six outputs", missing, rounds,
             steps), flush=True)
    times, sums = {}, {}
    for rnd in range(rounds):
        for pos, lib in enumerate(libs):
            path, _, route = lib.partition("@")
            env = dict(os.environ, METRAN_HIP_LIBRARY=os.path.abspath(path))
            out = subprocess.run([sys.executable, "-c", CHILD, str(B), str(T), "1" if sym else "0", "1" if filtered else "0", str(steps),
                                  str(missing), route or "default"], env=env, capture_output=True, text=True)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode != 0 or not line:
                print("%s (position %d, round %d) FAILED with exit status %d; nothing more is started\n%s"
                      % (lib, pos, rnd, out.returncode, out.stderr[-800:]), flush=True)
                return 1
            r = json.loads(line[0])
            tag = "%d:%s" % (pos, os.path.basename(lib))
            times.setdefault(tag, []).append((r["filter_ms"], r["smoother_ms"]))
            digest = " ".join("%s=%s" % kv for kv in sorted(r["chk"].items()))
            sums.setdefault(tag, set()).add((r["mle_sum"], digest))
            print("%-26s round %d  filter %.4f  smoother %.4f  mle_sum %.12e  %s" % (tag, rnd, r["filter_ms"], r["smoother_ms"], r["mle_sum"], digest),
                  flush=True)
    print("-- mean over the rounds (min .. max)")
    for tag, t in times.items():
        f, s = [x[0] for x in t], [x[1] for x in t]
        print("%-26s filter %.4f (%.4f .. %.4f)  smoother %.4f (%.4f .. %.4f)  outputs %s"
              % (tag, sum(f) / len(f), min(f), max(f), sum(s) / len(s), min(s), max(s),
                 "the same in every round" if len(sums[tag]) == 1 else "DIFFER between rounds"))
    every = set().union(*sums.values())
    print("-- outputs of all libraries: %s" % ("bit-identical" if len(every) == 1 else "%d different sets (timing builds differ by design)" % len(every)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
