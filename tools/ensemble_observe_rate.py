"""What observers cost an ensemble's stepping ("Ensembles": observers).

The shipped FHN 400 x 1600 and Goldbeter 100 x 400 grids in fp64, B = 16 members that differ in beta (tools/ensemble_rate.py's members):
ms per member-step with no observer, and with one open at stride 1, 10 and 100, statistics only and with maps.  Each figure is the
median over --batches batches of --steps steps, device-synchronised, after a warm-up batch; the spread is (max - min) / median over the
batches.  A sampling pass reads 16 B per point where a step moves 32: stride 1 is expected near +50 % where the members do not fit the
cache, stride >= 10 within a few per cent.

    python tools/ensemble_observe_rate.py [--members 16] [--steps 200] [--batches 9] [--out profiles/ensemble/observe_rate.txt]

--extras measures the sections and the cycle maps instead (profiles/ensemble/observe_sections_rate.txt): at each stride an observer
without extras, then the same observer with one column section, with both means, and with the cycle maps, each against the observer
without extras at that stride.  The sections launch reads 16 B per point for each of the two means (nothing to speak of for a column)
and writes 16 B per value of a line; the cycle maps add, per point and sample, a read and a write of the previous value (16 B) to the
sampling pass, and the three other planes only where a crossing falls.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crdmodel_amd as crd  # noqa: E402
from tools.ensemble_rate import members_of  # noqa: E402


def batches_ms(e, dt, steps, batches):
    out = []
    e.step_rk4(0.0, dt, steps, sync=True)  # warm-up
    for _ in range(batches):
        t = time.perf_counter()
        e.step_rk4(0.0, dt, steps, sync=True)
        out.append(1e3 * (time.perf_counter() - t))
    return out


def measure_extras(case, n, steps, batches, emit):
    members = members_of(case, n)
    g = crd.grid_of(members[0])
    dt = 0.004 if case == "fhn" else 0.002
    y0 = [crd.initial_conditions(crd.run_config(m)) for m in members]
    extras = [("no extras", {}), ("column section", {"sections": [("column", g.nx // 2)]}), ("both means", {"sections": [("theta_mean",), ("phi_mean",)]}),
              ("cycle maps", {"cycles": True, "cycle_threshold": 0.0})]
    for stride in (1, 10, 100):
        base = None
        for name, kw in extras:
            with crd.Ensemble(members) as e:
                for k, y in enumerate(y0):
                    e.upload(k, y)
                e.observe(stride=stride, probes=[(0, 0), (g.nx // 2, g.ny // 2)], capacity=(batches + 1) * (steps // stride + 1), **kw)
                ms = batches_ms(e, dt, steps, batches)
            med = statistics.median(ms)
            per = med / steps / n
            if base is None:
                base = per
            emit("%-9s %4dx%-4d B=%2d  stride %-3d %-15s %.5f ms/member-step  (batch %.2f ms, spread %.1f %%)  %+6.1f %% vs no extras" % (
                case, g.nx, g.ny, n, stride, name, per, med, 100.0 * (max(ms) - min(ms)) / med, 100.0 * (per / base - 1.0)))


def measure(case, n, steps, batches, emit):
    members = members_of(case, n)
    g = crd.grid_of(members[0])
    dt = 0.004 if case == "fhn" else 0.002
    y0 = [crd.initial_conditions(crd.run_config(m)) for m in members]
    configs = [("no observer", None, False)] + [("stride %d%s" % (s, ", maps" if m else ""), s, m) for m in (False, True) for s in (1, 10, 100)]
    base = None
    for name, stride, maps in configs:
        with crd.Ensemble(members) as e:
            for k, y in enumerate(y0):
                e.upload(k, y)
            blocks = 0
            if stride is not None:
                # (room for the warm-up and every batch)
                blocks = e.observe(stride=stride, probes=[(0, 0), (g.nx // 2, g.ny // 2)], maps=maps, threshold=0.0, capacity=(batches + 1) * (steps // stride + 1))["blocks_per_member"]
            ms = batches_ms(e, dt, steps, batches)
        med = statistics.median(ms)
        per = med / steps / n
        if base is None:
            base = per
        emit("%-9s %4dx%-4d B=%2d  %-18s %.5f ms/member-step  (batch %.2f ms, spread %.1f %%, G = %d)  %+6.1f %% vs no observer" % (
            case, g.nx, g.ny, n, name, per, med, 100.0 * (max(ms) - min(ms)) / med, blocks, 100.0 * (per / base - 1.0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--cases", default="fhn,goldbeter")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--extras", action="store_true", help="the sections and the cycle maps, against an observer without them")
    a = ap.parse_args()
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for case in a.cases.split(","):
        (measure_extras if a.extras else measure)(case, a.members, a.steps, a.batches, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
