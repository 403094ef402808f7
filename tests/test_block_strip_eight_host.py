"""The theta cut of the block-strip kernels for blocks of four and of eight wavefronts, in plain Python mirroring the host code
(crd_fused_plan.h: strip_count for the strip count; crd_fused_impl.h: fused_item_multi_step for x0, place, span and lane_stores): every column
of the grid is stored exactly once, for every nx from 64 to 2048.  And the set of widths at which a wavefront of the last block holds
only parked lanes, derived from x0 -- what tests/test_gpu_block_strip_eight.py takes its hazard widths from.

Beside it, the records of the eight-wide launch plans (chunk mode 3): profiles/pmc_traffic.json and plan_stats.json must have an entry
for each, stamped with the digest of the eight-wide kernel's own row of the build's kernel table."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, APRON = 64, 12  # three steps per launch: 3 x kApron columns a side


def theta_cut(nx, waves):
    """[(x0, [storing lanes])] of every wavefront of every block strip."""
    valid = waves * LANES - 2 * APRON
    blocks = (nx + valid - 1) // valid
    out = []
    for sblk in range(blocks):
        for wave in range(waves):
            x0 = sblk * valid - APRON + wave * LANES
            span = waves * LANES
            lanes = [lane for lane in range(LANES) if APRON <= wave * LANES + lane < span - APRON and x0 + lane < nx]
            out.append((x0, lanes))
    return out


@pytest.mark.parametrize("waves,valid", ((4, 232), (8, 488)))
def test_every_column_is_stored_exactly_once(waves, valid):
    for nx in range(64, 2049):
        cut = theta_cut(nx, waves)
        assert len(cut) == waves * -(-nx // valid)
        stored = [0] * nx
        for x0, lanes in cut:
            for lane in lanes:
                assert 0 <= x0 + lane < nx  # (a storing lane's column is inside the row unwrapped: its load offset serves the store)
                stored[x0 + lane] += 1
        assert stored == [1] * nx, (nx, waves)
        # useful lanes of all issued ones
        assert sum(len(lanes) for _, lanes in cut) == nx


def test_issued_lane_fractions_of_the_headline_grids():
    for nx, waves, blocks, frac in ((8192, 4, 36, 0.889), (8192, 8, 17, 0.941), (4096, 4, 18, 0.889), (4096, 8, 9, 0.889)):
        cut = theta_cut(nx, waves)
        assert len(cut) == blocks * waves
        assert abs(nx / (len(cut) * LANES) - frac) < 5e-4


def parked_wavefronts(nx, waves):
    """Wavefronts of the last block without a storing lane."""
    return sum(1 for _, lanes in theta_cut(nx, waves)[-waves:] if not lanes)


def test_widths_at_which_wavefronts_hold_only_parked_lanes():
    # eight wide: with r = nx - 488 (blocks - 1) in 1 .. 488, wavefront w >= 1 is parked iff 64 w - 12 >= r
    for nx in range(24, 2049):
        r = nx - 488 * (-(-nx // 488) - 1)
        assert parked_wavefronts(nx, 8) == sum(1 for w in range(1, 8) if 64 * w - 12 >= r), nx
    runs = {}
    for r in range(1, 489):
        runs.setdefault(parked_wavefronts(r, 8), []).append(r)
    assert {k: (v[0], v[-1]) for k, v in runs.items()} == {7: (1, 52), 6: (53, 116), 5: (117, 180), 4: (181, 244), 3: (245, 308), 2: (309, 372), 1: (373, 436), 0: (437, 488)}
    assert parked_wavefronts(200, 8) == 4 and parked_wavefronts(489, 8) == 7 and parked_wavefronts(976, 8) == 0
    # four wide, for comparison: other residues (of 232)
    assert [parked_wavefronts(nx, 4) for nx in (40, 52, 53, 116, 117, 180, 181, 232, 233)] == [3, 3, 2, 2, 1, 1, 0, 0, 3]


def test_the_eight_wide_plans_have_records_of_their_own_kernel():
    import bench
    import crdmodel_amd as crd

    wide = crd.launch_plan_candidates(eight_wide=True)
    assert wide == [(3, 0, 1, 1, 3), (3, 1, 1, 1, 3), (3, 2, 1, 1, 3)]
    assert not [q for q in crd.launch_plan_candidates() if q[0] == 3]
    path = os.path.join(ROOT, "crdmodel_amd", "csrc", "build", "kernel_table.json")
    if not os.path.exists(path):
        pytest.skip("no kernel table beside the library (a build with KERNEL_TABLE=0)")
    rows = json.load(open(path))["kernels"]
    wide_rows = [k for k in rows if k.get("waves", 4) == 8]
    assert sorted((k["precision"], k["model"], k["absorb"], k["embed"], k["cols"], k["nt"], k["steps"]) for k in wide_rows) == [("f64", 0, 0, 0, 1, 0, 3), ("f64", 0, 0, 0, 1, 1, 3)]
    for k in wide_rows:
        assert k["vgprs"] <= 256 and k["scratch_bytes"] == 0 and k["exec_skipped_vmem"] == 0 and k["async_lds_read_hazards"] == 0 and k["wavefronts_per_simd"] == 2, k
        narrow = [q for q in rows if "waves" not in q and all(q[f] == k[f] for f in ("precision", "model", "absorb", "embed", "cols", "nt", "steps"))]
        assert len(narrow) == 1 and narrow[0]["loop"]["valu"] == k["loop"]["valu"] and narrow[0]["lds_bytes"] < k["lds_bytes"]
        assert crd.kernel_digest_of_table_row(k) != crd.kernel_digest_of_table_row(narrow[0])
    want = crd.kernel_digest_of_table_row([k for k in wide_rows if k["nt"] == 1][0])
    traffic = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    stats = json.load(open(os.path.join(ROOT, "profiles", "plan_stats.json")))
    for plan in wide:
        key = crd.plan_key("fhn", "f64", plan)
        assert key in traffic and key in stats, key
        rec = traffic[key]
        assert rec["kernel_digest"] == want and stats[key]["kernel_digest"] == want, (key, rec["kernel_digest"], want)
        assert 32.0 <= rec["bytes_per_point"] <= 1.6 * 32.0 and abs(rec["write_bytes_per_point"] - 16.0) <= 0.8, (key, rec)
        assert os.path.exists(os.path.join(ROOT, rec["source"]))
        assert stats[key]["sweep_trace_avg_us"] > 0 and stats[key]["bench_stats_calls"] >= 100
        assert abs(stats[key]["bench_stats_avg_us"] - 1e3 * stats[key]["bench_kernel_ms_events"]) <= 0.03 * stats[key]["bench_stats_avg_us"], stats[key]
        assert bench.measured_traffic(key, 1 << 20, want)[0] is not None
