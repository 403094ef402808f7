"""What the run recorder costs a large single context and a LOCAL group's stepping ("Run recorder").

FHN 8192 x 8192 in fp64 on one device.  Every time is the device's (event pairs of step_rk4_timed) over batches of --steps steps; the
configurations of one comparison take their batches in turn (A B C A B C ...), after one warm-up batch each, and a figure is the median
over --batches batches with the spread (max - min) / median.  The lines:

  no recorder        this build against a build of the parent commit (--parent LIB: each build in processes of its own, since a
                     process holds one libcrd; the processes alternate, parent first, and the parent runs twice so that its own
                     process-to-process spread is on record).  The launches are the same: expected inside that spread.
  one sample         (batch with a recorder at stride 6 - batch without) / samples, in batches of a multiple of 6 steps -- whatever the
                     launch plan takes per launch (1, 2 or 3 steps), both batches group their steps alike, so the difference is the
                     samples' --: statistics only, with maps and cycle maps, with the
                     theta-mean section -- against the parent's crd_state_observe + crd_state_section(theta-mean) on the same state (two
                     reads of the state and two synchronous calls, host clock), and against reading the state once at the device's
                     streaming rate (profiles/hbm_streams.json).
  stride 1 / 10 / 100  ms per step with statistics, one probe and one column section.
  3 slabs, stride 10   a LOCAL group of three slabs on the one device, with and without the recorder.

    python tools/recorder_rate.py [--nx 8192] [--steps 20] [--batches 7] [--parent tools/_variants/parent/libcrd.so] [--out profiles/recorder/rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def params(crd, nx):
    return crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=nx, t_boundary=0.0)


def summary(ms):
    med = statistics.median(ms)
    return med, 100.0 * (max(ms) - min(ms)) / med


def child(a):
    """One process on whatever library CRD_LIBRARY names: batches without a recorder, then the one-shot calls.  One JSON line."""
    import crdmodel_amd as crd

    if os.environ.get("CRD_LIBRARY"):  # an earlier build of the same ABI number: it has everything this process calls but the recorder
        for name in [k for k in crd._capi._SIGNATURES if k.startswith("crd_recorder_")]:
            del crd._capi._SIGNATURES[name]
    p = params(crd, a.nx)
    dt = 0.5 * crd._capi.lib().crd_stable_dt(crd._capi.C.byref(p))
    out = {}
    with crd.Slab(p) as slab:
        slab.upload(crd.initial_conditions(crd.run_config(p)))
        slab.plan_launches()
        slab.step_rk4_timed(0.0, dt, a.steps)
        out["batch_ms"] = [slab.step_rk4_timed(0.0, dt, a.steps)[0] for _ in range(a.batches)]
        slab.observe(), slab.section("theta_mean")
        calls = []
        for _ in range(a.batches):
            t = time.perf_counter()
            slab.observe()
            slab.section("theta_mean")
            calls.append(1e3 * (time.perf_counter() - t))
        out["observe_section_ms"] = calls
    print(json.dumps(out), flush=True)


def in_turn(runs, steps, batches, dt):
    """runs: [(name, target)].  One warm-up batch each, then `batches` rounds in turn.  {name: [ms per batch]}"""
    def batch(tgt):
        r = tgt.step_rk4_timed(0.0, dt, steps)
        return r[0] if isinstance(r, tuple) else max(s["ms_total"] for s in r)

    for _, tgt in runs:
        batch(tgt)
    ms = {name: [] for name, _ in runs}
    for _ in range(batches):
        for name, tgt in runs:
            ms[name].append(batch(tgt))
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nx", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--parent", default=None, help="libcrd.so of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    n, steps = a.nx, a.steps
    emit("FHN %d x %d fp64, batches of %d steps, median over %d batches (spread = (max - min) / median)" % (n, n, steps, a.batches))
    # ---- no recorder: builds in processes of their own, alternating ----
    order = [("parent", a.parent), ("this build", None), ("parent (again)", a.parent), ("this build (again)", None)] if a.parent else [("this build", None)]
    seen = {}
    for name, libpath in order:
        env = dict(os.environ)
        env.pop("CRD_LIBRARY", None)
        if libpath:
            env["CRD_LIBRARY"] = os.path.abspath(libpath)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nx", str(n), "--steps", str(steps), "--batches", str(a.batches)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("child on %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
        seen[name] = json.loads(r.stdout.strip().splitlines()[-1])
        med, spread = summary(seen[name]["batch_ms"])
        emit("no recorder        %-18s %.4f ms/step  (batch %.3f ms, spread %.1f %%)" % (name, med / steps, med, spread))
    if a.parent:
        pa, pb = summary(seen["parent"]["batch_ms"])[0], summary(seen["parent (again)"]["batch_ms"])[0]
        ta = statistics.median(seen["this build"]["batch_ms"] + seen["this build (again)"]["batch_ms"])
        emit("no recorder        parent against parent %+.2f %%; this build against the parents' mean %+.2f %%" % (100.0 * (pb / pa - 1.0), 100.0 * (ta / (0.5 * (pa + pb)) - 1.0)))
        med, spread = summary(seen["parent"]["observe_section_ms"] + seen["parent (again)"]["observe_section_ms"])
        emit("parent             crd_state_observe + crd_state_section(theta-mean): %.3f ms per pair of calls (host clock, spread %.1f %%)" % (med, spread))
        parent_pair = med
    streams = json.load(open(os.path.join(ROOT, "profiles", "hbm_streams.json")))
    state_bytes = 2.0 * 8.0 * n * n
    emit("streaming          reading the state once (%.2f GB) at %d GB/s (profiles/hbm_streams.json): %.3f ms" % (state_bytes / 1e9, streams["read_only_gbs"], state_bytes / streams["read_only_gbs"] / 1e6))

    import crdmodel_amd as crd

    p = params(crd, n)
    dt = 0.5 * crd._capi.lib().crd_stable_dt(crd._capi.C.byref(p))
    y0 = crd.initial_conditions(crd.run_config(p))
    room = (a.batches + 1) * (steps + 6)

    def lone(**kw):
        slab = crd.Slab(p)
        slab.upload(y0)
        slab.plan_launches()
        rec = crd.Recorder(slab, capacity=room, **kw) if kw else None
        return slab, rec

    # ---- the sample pass alone ----
    kinds = [("statistics only", dict(stride=6)), ("maps and cycle maps", dict(stride=6, maps=True, threshold=0.0, cycles=True, cycle_threshold=0.0)),
             ("theta-mean section", dict(stride=6, sections=[("theta_mean",)]))]
    steps6 = 6 * ((steps + 5) // 6)
    for name, kw in kinds:
        (plain, _), (seen_slab, rec) = lone(), lone(**kw)
        ms = in_turn([("plain", plain), ("recorded", seen_slab)], steps6, a.batches, dt)
        diffs = [(r - q) / (steps6 // 6) for q, r in zip(ms["plain"], ms["recorded"])]
        med = statistics.median(diffs)
        emit("one sample         %-20s %.3f ms  (spread %.1f %% of it; plain step %.4f ms)%s" % (
            name, med, 100.0 * (max(diffs) - min(diffs)) / med, statistics.median(ms["plain"]) / steps6,
            "  = %.2f x the parent's two calls" % (med / parent_pair) if a.parent and name != "maps and cycle maps" else ""))
        rec.close(), plain.close(), seen_slab.close()
    # ---- strides ----
    runs = [("no recorder", lone())] + [("stride %d" % s, lone(stride=s, probes=[(n // 2, n // 2)], sections=[("column", n // 2)])) for s in (1, 10, 100)]
    ms = in_turn([(name, sr[0]) for name, sr in runs], steps, a.batches, dt)
    base = statistics.median(ms["no recorder"]) / steps
    for name, _ in runs:
        med, spread = summary(ms[name])
        emit("per step           %-12s %.4f ms/step  (spread %.1f %%)  %+6.1f %% vs no recorder" % (name, med / steps, spread, 100.0 * (med / steps / base - 1.0)))
    for _, (slab, rec) in runs:
        slab.close()
    # ---- a LOCAL group of three slabs on the one device ----
    groups = []
    for recorded in (False, True):
        g = crd.LocalGroup(p, 3)
        g.upload(y0)
        for s in g.slabs:
            s.plan_launches()
        if recorded:
            recorders = [crd.Recorder(g, stride=10, probes=[(n // 2, n // 2)], sections=[("column", n // 2)], capacity=room)]
        groups.append(("stride 10" if recorded else "no recorder", g))
    ms = in_turn(groups, steps, a.batches, dt)
    base = statistics.median(ms["no recorder"]) / steps
    for name, _ in groups:
        med, spread = summary(ms[name])
        emit("3 slabs, 1 device  %-12s %.4f ms/step  (spread %.1f %%)  %+6.1f %% vs no recorder" % (name, med / steps, spread, 100.0 * (med / steps / base - 1.0)))
    del recorders
    for _, g in groups:
        g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
