"""The oracle and libcrd's host side against TWO- and FOUR-rank runs of the reference's OWN compiled code (tests/golden/refranks_*.npz).

The fixtures hold what the reference's four programs, compiled unmodified against the stand-in headers of oracle/ref_build/, wrote when
run as 1, 2 and 4 rank processes side by side (oracle/ref_build/make_rank_fixtures.py; the stand-in mpi.h carries their messages
through a directory): per rank the subdomain line, the initial row, f() on the rank's block of given states -- with the halos its own
Exchange() received from the other ranks -- and, for one case, a fixed-step RK4 run.  MPI_Dims_create gives {2, 1} for two ranks (two
theta-blocks of full height, not two phi-slabs) and {2, 2} for four.  Everything is compared bit for bit; no tolerance anywhere.

What stands on these files: crd_dims_create, crd_block_extents, the rank order c0 d1 + c1, block initial conditions, the block file
sets of crd.Writer(block=...), the oracle's subproblem / halo strips -- and the reference's own decomposition invariance, which the
project had so far only restated.  Each check is also handed a planted fault (one ulp in an edge column of one block, the rank map
transposed, west and east halos swapped) and has to fail.

Not pinned: ARKode's adaptive step sequence; three or more ranks in a direction stay outside (the reference's
exchange is the periodic halo only up to two).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from oracle import crd_oracle as co
from oracle.ref_build import build_ref
from oracle.ref_build import make_fixtures as mf
from oracle.ref_build import make_rank_fixtures as mr
from test_refprobe_host import need_compiled_reference, require_bits

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = [os.path.basename(p)[len(mr.PREFIX):-4] for p in mr.fixture_paths()]
PROBE = [t for t in TAGS if not t.startswith("rk4_")]
RK4 = [t for t in TAGS if t.startswith("rk4_")]
KEPT = ["fhn_torus_13_vb", "gb_torus_13"]  # the two smallest (13 x 19) hold the complete text files
RANKS = mr.RANKS

# THE CASE TABLE of rows that differ between rank counts BY THE REFERENCE'S OWN RULE (everything else is the cut of the one-rank rows).
# tag -> the frames concerned and the relation asserted in place of equality.
#   gb_flat_13_vb_ic2, frame 0 (the initial row): icType = 2 draws (float) rand() / RAND_MAX * 1.4 point by point and never calls
#   srand(); every rank is a process of its own, so each draws the SAME sequence over its own points: a rank's initial row is the
#   first 2 nxl nyl values of the one-rank initial row.  Its f() rows are cuts like everyone's (the probe state is handed in).
OWN_ROWS = {"gb_flat_13_vb_ic2": (0,)}
_cache = {}


class Rank:
    """What one rank of an n-rank run wrote: its subdomain line, its extents as that line states them, its rows (frames, nyl, nxl, 2)."""

    def __init__(self, header, var0, var1):
        self.header = header
        self.nx, self.ny, self.is_, self.ie, self.js, self.je = mr.extents_of(header)
        self.nxl, self.nyl = self.ie - self.is_ + 1, self.je - self.js + 1
        self.rows = np.stack([var0, var1], axis=-1).reshape(var0.shape[0], self.nyl, self.nxl, 2)

    def cut(self, whole):
        """This rank's block of a (..., ny, nx, 2) array."""
        return whole[..., self.js:self.je + 1, self.is_:self.ie + 1, :]


class Fixture:
    def __init__(self, tag):
        self.tag = tag
        d = np.load(os.path.join(mf.GOLDEN, mr.PREFIX + tag + ".npz"), allow_pickle=False)
        self.d = {k: d[k] for k in d.files}
        self.program = str(self.d["program"])
        self.cfg, self.op = mf.load(str(self.d["ini_text"]), self.program)
        self.cfg.steady_state_decimals = 8  # the route the reference takes: the printed line (Goldbeter; no effect on FHN)
        self.steady = tuple(float(v) for v in self.d["steady_line"]) or None
        self.one = self.ranks(1)[0].rows  # (frames, ny, nx, 2)

    def ranks(self, n):
        """The n ranks in rank order; each takes its values from the shared arrays by the size ITS OWN header states."""
        headers = [bytes(h) for h in self.d["header_np%d" % n]]
        assert len(headers) == n, (self.tag, n)
        out, at = [], 0
        for h in headers:
            e = mr.extents_of(h)
            m = (e[3] - e[2] + 1) * (e[5] - e[4] + 1)
            out.append(Rank(h, self.d["var0_np%d" % n][:, at:at + m], self.d["var1_np%d" % n][:, at:at + m]))
            at += m
        assert at == self.d["var0_np%d" % n].shape[1] == self.op.nx * self.op.ny, (self.tag, n, at)
        return out

    def probes(self):
        for k, (t, s) in enumerate(zip(self.d["probe_t"], self.d["probe_state"])):
            yield k, float(t), self.d["states"][s].astype(np.float64), str(self.d["state_names"][s])


def fixture(tag):
    if tag not in _cache:
        _cache[tag] = Fixture(tag)
    return _cache[tag]


def row_major(c0, c1, d0, d1):
    """MPI_Cart_create with reorder = 0, and the project's rank order."""
    return c0 * d1 + c1


def transposed(c0, c1, d0, d1):
    """The planted fault: the map the other way round."""
    return c1 * d0 + c0


def blocks_of(n):
    """[(c0, d0, c1, d1)] of crd.dims_create(n), in the order the project numbers them."""
    d0, d1 = crd.dims_create(n)
    return [(c0, d0, c1, d1) for c0 in range(d0) for c1 in range(d1)]


# ---- the checks (each takes the ranks as an argument, so that the planted tests can hand it moved ones) ----------------------------

def check_invariance(fx, n, ranks):
    """The reference's own decomposition invariance: the ranks' rows, placed by the extents in their own headers, are the one-rank rows."""
    cover = np.zeros((fx.op.ny, fx.op.nx), dtype=int)
    for r in ranks:
        assert (r.nx, r.ny) == (fx.op.nx, fx.op.ny), (fx.tag, n, r.header)
        cover[r.js:r.je + 1, r.is_:r.ie + 1] += 1
    assert np.all(cover == 1), "%s: the %d ranks' extents do not tile the grid" % (fx.tag, n)
    for frame in range(fx.one.shape[0]):
        if frame in OWN_ROWS.get(fx.tag, ()):
            for k, r in enumerate(ranks):  # every rank draws the one sequence over its own points
                got, ref = r.rows[frame].ravel(), fx.one[frame].ravel()[:2 * r.nxl * r.nyl]
                assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), "%s: rank %d of %d does not draw the one-rank sequence" % (fx.tag, k, n)
                if n > 1 and (r.nxl < fx.op.nx):
                    assert not np.array_equal(r.rows[frame], r.cut(fx.one[frame])), (fx.tag, k, n)  # ... which is NOT the cut
            continue
        stitched = np.full_like(fx.one[frame], np.nan)
        for r in ranks:
            stitched[r.js:r.je + 1, r.is_:r.ie + 1] = r.rows[frame]
        require_bits("%s frame %d: the %d ranks' rows against the one-rank row" % (fx.tag, frame, n), stitched, fx.one[frame])


def check_extents(fx, n, ranks, rank_of=row_major):
    """crd.dims_create, crd.block_extents and the oracle's subproblem with rank = c0 d1 + c1 against every header's is ie js je."""
    for c0, d0, c1, d1 in blocks_of(n):
        r = ranks[rank_of(c0, c1, d0, d1)]
        want = (r.is_, r.ie, r.js, r.je)
        assert crd.block_extents(fx.op.nx, fx.op.ny, c0, d0, c1, d1) == want, ("crd.block_extents", fx.tag, n, (c0, c1), r.header)
        sub = co.subproblem(fx.op, d0, d1, c0, c1)
        assert (sub.is_, sub.ie, sub.js, sub.je) == want, ("co.subproblem", fx.tag, n, (c0, c1), r.header)


def check_initial_conditions(fx, n, ranks, rank_of=row_major):
    if fx.steady is not None:
        assert crd.steady_state_as_printed("goldbeter", fx.cfg.params.beta, 8) == fx.steady, (fx.tag, fx.steady)
    cfg = fx.cfg
    for c0, d0, c1, d1 in blocks_of(n):
        k = rank_of(c0, c1, d0, d1)
        is_, ie, js, je = crd.block_extents(fx.op.nx, fx.op.ny, c0, d0, c1, d1)
        require_bits("%s rank %d of %d: crd.initial_conditions" % (fx.tag, k, n), crd.initial_conditions(cfg, js, je, is_, ie), ranks[k].rows[0])
        got = co.initial_conditions(co.subproblem(fx.op, d0, d1, c0, c1), cfg.wave_length, cfg.wave_width, cfg.wave_inside, cfg.ic_type, steady_state=fx.steady)
        require_bits("%s rank %d of %d: co.initial_conditions" % (fx.tag, k, n), got, ranks[k].rows[0])


def check_files(fx, n, ranks, directory, whole_files):
    """crd.Writer(block=...) writes each rank's subdomain file byte for byte (xmin xmax tfinal included), and from the parsed rows the
    complete field files where the fixture kept them."""
    names = mf.PROGRAMS[fx.program][3]
    for c0, d0, c1, d1 in blocks_of(n):
        k = row_major(c0, c1, d0, d1)
        with crd.Writer(fx.cfg, directory, block=(c0, d0, c1, d1)) as w:
            for row in (ranks[k].rows if whole_files else ()):
                w.write_row(row)
        with open(os.path.join(directory, "%s_subdomain.%03d.txt" % (fx.program, k)), "rb") as f:
            assert f.read() == ranks[k].header, (fx.tag, n, k, ranks[k].header)
        for v, name in enumerate(names if whole_files else ()):
            with open(os.path.join(directory, "%s_%s.%03d.txt" % (fx.program, name, k)), "rb") as f:
                got = f.read()
            assert got == fx.d["file_np%d_rank%d_var%d" % (n, k, v)].tobytes(), "%s: %s_%s.%03d.txt differs from the reference's file" % (fx.tag, fx.program, name, k)
    assert not os.path.exists(os.path.join(directory, "%s_subdomain.%03d.txt" % (fx.program, n)))


def block_rhs(fx, n, t, parts, swap_halos=False):
    """f() block by block as tests/test_oracle.py builds it: co.subproblem, the four strips of co.pack_edges of every block, each block
    evaluated by co.rhs_subdomain with the strips its periodic neighbours sent: from the west neighbour its last column, from the east
    its first, from the south its last row, from the north its first.  parts: the blocks' states in rank order."""
    blocks = blocks_of(n)
    subs = [co.subproblem(fx.op, d0, d1, c0, c1) for c0, d0, c1, d1 in blocks]
    sent = [co.pack_edges(s, y) for s, y in zip(subs, parts)]  # (w = last column, e = first column, s = last row, n = first row)
    out = []
    for (c0, d0, c1, d1), sub, y in zip(blocks, subs, parts):
        west, east = row_major((c0 - 1) % d0, c1, d0, d1), row_major((c0 + 1) % d0, c1, d0, d1)
        south, north = row_major(c0, (c1 - 1) % d1, d0, d1), row_major(c0, (c1 + 1) % d1, d0, d1)
        wrecv, erecv = sent[west][0], sent[east][1]
        if swap_halos:
            wrecv, erecv = erecv, wrecv
        out.append(co.rhs_subdomain(sub, t, y, wrecv, erecv, sent[south][2], sent[north][3]))
    return out


def check_block_rhs(fx, n, ranks, swap_halos=False):
    """The oracle through its block decomposition gives each rank's f() rows."""
    for k, t, y, name in fx.probes():
        got = block_rhs(fx, n, t, [np.ascontiguousarray(r.cut(y)) for r in ranks], swap_halos)
        for q, r in enumerate(ranks):
            require_bits("%s probe %d (%s state, t = %g), rank %d of %d: co.rhs_subdomain" % (fx.tag, k, name, t, q, n), got[q], r.rows[k + 1])


def output_times(fx):
    """(t, tout, steps) of the reference's output loop: tout += dTout, capped at tFinal."""
    cfg, dt = fx.cfg, float(fx.d["dt"])
    d_out = cfg.t_final / cfg.output_timestep
    t, tout = 0.0, d_out
    for _ in range(cfg.output_timestep):
        yield t, tout, int(round((tout - t) / dt))
        t, tout = tout, min(tout + d_out, cfg.t_final)


def check_block_rk4(fx, n, ranks, swap_halos=False):
    """Classical RK4 on the blocks, every stage through block_rhs, the stage states and the update in the operation order of
    crd_oracle_rk4 (= the stand-in ARKode's fixed-step mode): each rank's output rows."""
    dt = float(fx.d["dt"])
    y = [np.array(r.rows[0]) for r in ranks]
    for k, (t0, tout, steps) in enumerate(output_times(fx), start=1):
        assert steps == int(fx.d["steps_per_output"]), (fx.tag, k, steps)
        for s in range(steps):
            t = t0 + float(s) * dt
            k1 = block_rhs(fx, n, t, y, swap_halos)
            k2 = block_rhs(fx, n, t + 0.5 * dt, [a + (0.5 * dt) * b for a, b in zip(y, k1)], swap_halos)
            k3 = block_rhs(fx, n, t + 0.5 * dt, [a + (0.5 * dt) * b for a, b in zip(y, k2)], swap_halos)
            k4 = block_rhs(fx, n, t + dt, [a + dt * b for a, b in zip(y, k3)], swap_halos)
            y = [a + (dt / 6.0) * (b1 + 2.0 * b2 + 2.0 * b3 + b4) for a, b1, b2, b3, b4 in zip(y, k1, k2, k3, k4)]
        for q, r in enumerate(ranks):
            require_bits("%s output %d (t = %.17g), rank %d of %d: RK4 through co.rhs_subdomain" % (fx.tag, k, tout, q, n), y[q], r.rows[k])


# ---- the fixtures as committed -----------------------------------------------------------------------------------------------------

def test_every_case_has_its_fixture():
    assert sorted(TAGS) == sorted(c["tag"] for c in mr.CASES)
    sizes = [os.path.getsize(p) for p in mr.fixture_paths()]
    assert max(sizes) <= mr.MAX_FIXTURE_BYTES and sum(sizes) < mr.MAX_TOTAL_BYTES == 600000, (max(sizes), sum(sizes))
    assert {t for t in TAGS if str(fixture(t).d["own_rows"])} == set(OWN_ROWS)  # the case table above is the fixtures'
    assert [t for t in TAGS if "file_np4_rank3_var1" in fixture(t).d] == sorted(KEPT)
    programs = {fixture(t).program for t in TAGS}
    assert programs == set(mf.PROGRAMS)
    odd = {str(fixture(t).d["surface"]) for t in TAGS if fixture(t).op.nx % 2 and fixture(t).op.ny % 2}
    assert odd == {"torus", "flat"}  # nx c / d and ny c / d truncate on both surfaces
    # what tests/test_gpu_refranks.py asks of the grids: 8 rows per block of 2 x 2; four phi-slabs of 12 rows for the RK4 run
    assert all(fixture(t).op.ny >= 16 for t in TAGS) and all(fixture(t).op.ny >= 48 for t in RK4)


def test_two_ranks_are_two_theta_blocks_and_four_are_two_by_two():
    """MPI_Dims_create as the reference's runs show it: np = 2 splits theta (columns) and leaves phi whole."""
    for tag in TAGS:
        fx = fixture(tag)
        two, four = fx.ranks(2), fx.ranks(4)
        assert [(r.js, r.je) for r in two] == [(0, fx.op.ny - 1)] * 2 and two[0].ie + 1 == two[1].is_ == fx.op.nx // 2
        assert [(r.is_, r.js) for r in four] == [(0, 0), (0, fx.op.ny // 2), (fx.op.nx // 2, 0), (fx.op.nx // 2, fx.op.ny // 2)]


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", TAGS)
def test_the_reference_is_invariant_under_its_own_decomposition(tag, n):
    fx = fixture(tag)
    check_invariance(fx, n, fx.ranks(n))


@pytest.mark.parametrize("n", (1,) + RANKS)
@pytest.mark.parametrize("tag", TAGS)
def test_dims_extents_and_rank_order_are_the_headers(tag, n):
    fx = fixture(tag)
    assert crd.dims_create(n) == {1: (1, 1), 2: (2, 1), 4: (2, 2)}[n]
    check_extents(fx, n, fx.ranks(n))


@pytest.mark.parametrize("n", (1,) + RANKS)
@pytest.mark.parametrize("tag", TAGS)
def test_block_initial_conditions_are_each_ranks_first_row(tag, n):
    fx = fixture(tag)
    check_initial_conditions(fx, n, fx.ranks(n))


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", TAGS)
def test_writer_reproduces_each_ranks_files(tag, n, tmp_path):
    fx = fixture(tag)
    check_files(fx, n, fx.ranks(n), str(tmp_path), tag in KEPT)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", PROBE)
def test_oracle_blocks_with_halos_are_each_ranks_f(tag, n):
    fx = fixture(tag)
    check_block_rhs(fx, n, fx.ranks(n))


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", RK4)
def test_oracle_blocks_rk4_is_each_ranks_run(tag, n):
    fx = fixture(tag)
    check_block_rk4(fx, n, fx.ranks(n))


def test_host_abi_block_of_the_whole_field_claim_holds_where_it_is_made():
    """tests/test_host_abi.py::test_block_decomposition_follows_setupdecomp says a block's initial conditions are the block of the whole
    field, for the four rules it lists; the reference's ranks agree for every rule but rand() (OWN_ROWS), which that test does not list
    and for which the project draws block by block as the ranks do."""
    for tag in TAGS:
        fx = fixture(tag)
        whole = crd.initial_conditions(fx.cfg)
        for n in RANKS:
            for r in fx.ranks(n):
                same = np.array_equal(crd.initial_conditions(fx.cfg, r.js, r.je, r.is_, r.ie), r.cut(whole))
                assert same == (tag not in OWN_ROWS), (tag, n, r.header)


# ---- every check bites -------------------------------------------------------------------------------------------------------------

def edge_points(r):
    """(row, column) in a block: its first and last column (the theta seams between blocks), first, middle and last row."""
    return [(0, 0), (r.nyl // 2, r.nxl - 1), (r.nyl - 1, 0), (r.nyl - 1, r.nxl - 1)]


def with_moved(ranks, q, frame, row, col, field):
    """The ranks with one value of rank q moved to the next double."""
    out = [Rank(r.header, r.rows[..., 0].reshape(r.rows.shape[0], -1), r.rows[..., 1].reshape(r.rows.shape[0], -1)) for r in ranks]
    out[q].rows = out[q].rows.copy()
    out[q].rows[frame, row, col, field] = np.nextafter(out[q].rows[frame, row, col, field], np.inf)
    return out


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", ["fhn_torus_23x57", "gb_flat_13x39", "gb_flat_13_vb_ic2"])
def test_planted_ulp_in_an_edge_column_fails_every_row_check(tag, n):
    fx = fixture(tag)
    ranks = fx.ranks(n)
    for q in (0, n - 1):
        for point, (j, i) in enumerate(edge_points(ranks[q])):
            field = point % 2
            for frame in range(fx.one.shape[0]):
                bad = with_moved(ranks, q, frame, j, i, field)
                with pytest.raises(AssertionError):
                    check_invariance(fx, n, bad)
                where = r"rank %d of %d.*field %d differs at 1 point\(s\), first at \(row %d, column %d\)" % (q, n, field, j, i)
                with pytest.raises(AssertionError, match=where):
                    check_initial_conditions(fx, n, bad) if frame == 0 else check_block_rhs(fx, n, bad)


@pytest.mark.parametrize("n", RANKS)
def test_planted_ulp_fails_the_rk4_and_file_checks(n, tmp_path):
    fx = fixture(RK4[0])
    ranks = fx.ranks(n)
    for q in (0, n - 1):
        j, i = edge_points(ranks[q])[1]
        for frame in (1, fx.one.shape[0] - 1):
            with pytest.raises(AssertionError, match=r"output %d .*rank %d of %d.*\(row %d, column %d\)" % (frame, q, n, j, i)):
                check_block_rk4(fx, n, with_moved(ranks, q, frame, j, i, frame % 2))
    fx = fixture(KEPT[0])
    ranks = fx.ranks(n)
    j, i = edge_points(ranks[n - 1])[1]
    with pytest.raises(AssertionError, match="differs from the reference's file"):
        check_files(fx, n, with_moved(ranks, n - 1, fx.one.shape[0] - 1, j, i, 1), str(tmp_path), True)


@pytest.mark.parametrize("tag", TAGS)
def test_transposed_rank_map_fails_on_four_ranks(tag):
    """(c0, c1) -> c1 d0 + c0 exchanges ranks 1 and 2 of the 2 x 2 grid: their extents differ, and so do their initial rows."""
    fx = fixture(tag)
    ranks = fx.ranks(4)
    with pytest.raises(AssertionError, match="crd.block_extents"):
        check_extents(fx, 4, ranks, rank_of=transposed)
    if ranks[1].rows[0].shape != ranks[2].rows[0].shape or not np.array_equal(ranks[1].rows[0], ranks[2].rows[0]):
        with pytest.raises(AssertionError):
            check_initial_conditions(fx, 4, ranks, rank_of=transposed)
    check_extents(fx, 2, fx.ranks(2), rank_of=transposed)  # (2 x 1: the two maps coincide, nothing to tell apart)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", PROBE + RK4)
def test_swapped_west_and_east_halos_fail(tag, n):
    fx = fixture(tag)
    with pytest.raises(AssertionError, match="co.rhs_subdomain"):
        (check_block_rk4 if tag in RK4 else check_block_rhs)(fx, n, fx.ranks(n), swap_halos=True)


def test_a_wrong_subdomain_line_fails_the_file_check(tmp_path):
    fx = fixture("fhn_torus_23x57")
    ranks = fx.ranks(4)
    check_files(fx, 4, ranks, str(tmp_path), False)
    for k, wrong in ((2, b"12"), (5, b"57"), (7, b"6.283186"), (8, b"1.200001")):  # is, je, xmax, tFinal of rank 3
        words = ranks[3].header.split()
        words[k] = wrong
        bad = list(ranks)
        bad[3] = Rank(ranks[3].header, ranks[3].rows[..., 0].reshape(ranks[3].rows.shape[0], -1), ranks[3].rows[..., 1].reshape(ranks[3].rows.shape[0], -1))
        bad[3].header = b"  ".join(words[:6]) + b" " + b" ".join(words[6:]) + b"\n"
        with pytest.raises(AssertionError):
            check_files(fx, 4, bad, str(tmp_path), False)


# ---- the fixtures are what the recipe makes ----------------------------------------------------------------------------------------

def test_rank_fixtures_regenerate_from_the_compiled_reference(tmp_path):
    """With oracle/_ref/ built: run the recipe again and require the committed contents, array by array."""
    need_compiled_reference()
    if not build_ref.current() and build_ref.reference_dir() is None:
        pytest.skip("oracle/_ref/ was compiled against earlier stand-in headers (a one-rank mpi.h) and no reference tree is here to compile it again")
    mr.make_all(str(tmp_path))  # (compiles oracle/_ref/ again first where it is older than the stand-in headers)
    made = [os.path.basename(p) for p in mr.fixture_paths(str(tmp_path))]
    assert made == [os.path.basename(p) for p in mr.fixture_paths()]
    for name in made:
        new, old = np.load(os.path.join(str(tmp_path), name), allow_pickle=False), np.load(os.path.join(mf.GOLDEN, name), allow_pickle=False)
        assert sorted(new.files) == sorted(old.files), name
        for k in new.files:
            if k == "provenance":  # the compiler's version line may differ between machines; the sources and flags may not
                a, b = json.loads(str(new[k])), json.loads(str(old[k]))
                assert (a["sources"], a["flags"]) == (b["sources"], b["flags"]), name
                continue
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)


# ---- the stand-in mpi.h by itself: a small program compiled against the header -----------------------------------------------------

RANK_PROGRAM = r"""
#include <mpi.h>
/* argv: mode, doubles to send, doubles to receive.  Two messages go to the +1 neighbour of dimension 0 and two are received from the
 * -1 neighbour with MPI_ANY_TAG; the received values are printed in the order of the receives. */
int main(int argc, char **argv)
{
	const char *mode = argv[1];
	const int nsend = atoi(argv[2]), nrecv = atoi(argv[3]);
	int rank, size, dims[2] = {0, 0}, periods[2] = {1, 1}, coords[2], source, dest;
	MPI_Comm cart;
	MPI_Init(&argc, &argv);
	MPI_Comm_rank(MPI_COMM_WORLD, &rank);
	MPI_Comm_size(MPI_COMM_WORLD, &size);
	MPI_Dims_create(size, 2, dims);
	MPI_Cart_create(MPI_COMM_WORLD, 2, dims, periods, 0, &cart);
	MPI_Cart_get(cart, 2, dims, periods, coords);
	MPI_Cart_shift(cart, 0, 1, &source, &dest);
	printf("rank %d of %d dims %d %d coords %d %d source %d dest %d\n", rank, size, dims[0], dims[1], coords[0], coords[1], source, dest);
	fflush(stdout);
	double a[8], b[8], ra[8] = {0}, rb[8] = {0};
	for (int k = 0; k < 8; k++) a[k] = 100 * rank + k, b[k] = 100 * rank + 50 + k;
	MPI_Request sa, sb, qa, qb;
	MPI_Status st;
	if (strcmp(mode, "outside") == 0) MPI_Isend(a, nsend, MPI_DOUBLE, size, 0, cart, &sa);
	if (strcmp(mode, "leftover") == 0) {
		MPI_Isend(a, nsend, MPI_DOUBLE, rank, 0, cart, &sa);
		MPI_Wait(&sa, &st);
		MPI_Finalize();
		return 0;
	}
	MPI_Irecv(ra, nrecv, MPI_DOUBLE, source, MPI_ANY_TAG, cart, &qa);
	MPI_Irecv(rb, nrecv, MPI_DOUBLE, source, MPI_ANY_TAG, cart, &qb);
	MPI_Isend(a, nsend, MPI_DOUBLE, dest, 0, cart, &sa);
	MPI_Isend(b, nsend, MPI_DOUBLE, dest, 1, cart, &sb);
	MPI_Wait(&qb, &st); /* the second receive first: it still gets the second message */
	MPI_Wait(&qa, &st);
	MPI_Wait(&sa, &st);
	MPI_Wait(&sb, &st);
	if (strcmp(mode, "twice") == 0) MPI_Wait(&qa, &st);
	printf("received %g %g then %g %g\n", ra[0], ra[nrecv - 1], rb[0], rb[nrecv - 1]);
	if (strcmp(mode, "unwaited") == 0) MPI_Isend(a, nsend, MPI_DOUBLE, dest, 0, cart, &sa);
	MPI_Finalize();
	return 0;
}
"""


@pytest.fixture(scope="module")
def rank_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mpi_standin")
    (d / "rank_program.cpp").write_text(RANK_PROGRAM)
    exe = str(d / "rank_program")
    subprocess.run([os.environ.get("CXX", "g++"), "-O0", "-w", "-I", os.path.join(mr.HERE, "include"), str(d / "rank_program.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def run_rank_program(exe, directory, size, args, only=None, deadline="20"):
    """`size` processes side by side (only: just these ranks); returns [(returncode, stdout, stderr)] in rank order."""
    os.makedirs(directory, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CRD_REF_")}
    procs = []
    for k in (range(size) if only is None else only):
        e = dict(env, CRD_REF_MPI_SIZE=str(size), CRD_REF_MPI_RANK=str(k), CRD_REF_MPI_DIR=str(directory), CRD_REF_MPI_DEADLINE=deadline)
        procs.append(subprocess.Popen([exe] + [str(a) for a in args(k)], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=60)
            out.append((p.returncode, so, se))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return out


ABORTED = -6  # SIGABRT


def test_stand_in_mpi_carries_messages_in_order_between_rank_processes(rank_program, tmp_path):
    """The healthy run: grid, coordinates, periodic neighbours, and MPI's non-overtaking order under MPI_ANY_TAG."""
    for size, grid in ((2, [("2 1", "0 0", 1, 1), ("2 1", "1 0", 0, 0)]),
                       (4, [("2 2", "0 0", 2, 2), ("2 2", "0 1", 3, 3), ("2 2", "1 0", 0, 0), ("2 2", "1 1", 1, 1)])):
        d = tmp_path / ("np%d" % size)
        out = run_rank_program(rank_program, d, size, lambda k: ("exchange", 8, 8))
        for k, ((rc, so, se), (dims, coords, source, dest)) in enumerate(zip(out, grid)):
            assert rc == 0, (size, k, se)
            assert "rank %d of %d dims %s coords %s source %d dest %d\n" % (k, size, dims, coords, source, dest) in so, so
            assert "received %d %d then %d %d\n" % (100 * source, 100 * source + 7, 100 * source + 50, 100 * source + 57) in so, so
        assert os.listdir(d) == []  # every message received and removed
    # with no size in the environment the same program is the one-rank stand-in: both neighbours are rank 0 itself
    env = {k: v for k, v in os.environ.items() if not k.startswith("CRD_REF_")}
    r = subprocess.run([rank_program, "exchange", "8", "8"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "rank 0 of 1 dims 1 1 coords 0 0 source 0 dest 0\nreceived 0 7 then 50 57\n" == r.stdout, (r.stdout, r.stderr)


def test_stand_in_mpi_fails_the_way_the_library_would(rank_program, tmp_path):
    """Every way the multi-rank mode can go wrong aborts with a message: a size mismatch, a missing partner (at the deadline, here
    shortened through the environment), a second wait, a request or a message left at MPI_Finalize, a peer outside the grid, a size
    other than 2 or 4."""
    out = run_rank_program(rank_program, tmp_path / "size", 2, lambda k: ("exchange", 3 if k == 0 else 4, 4))
    assert out[1][0] == ABORTED and "MPI stand-in, rank 1 of 2: a matched send and receive differ in size" in out[1][2], out[1]
    assert out[0][0] == 0, out[0]  # (rank 0 got its four values; nothing is wrong on its side)
    (rc, so, se), = run_rank_program(rank_program, tmp_path / "lost", 2, lambda k: ("exchange", 4, 4), only=[0], deadline="0.2")
    assert rc == ABORTED and "rank 0 of 2: MPI_Wait: no message from the receive's source by the deadline" in se, (rc, se)
    out = run_rank_program(rank_program, tmp_path / "twice", 2, lambda k: ("twice", 4, 4))
    assert all(rc == ABORTED and "MPI_Wait twice on one request" in se for rc, _, se in out), out
    out = run_rank_program(rank_program, tmp_path / "unwaited", 2, lambda k: ("unwaited", 4, 4))
    assert all(rc == ABORTED and "a request was never waited for at MPI_Finalize" in se for rc, _, se in out), out
    (rc, so, se), = run_rank_program(rank_program, tmp_path / "leftover", 2, lambda k: ("leftover", 4, 4), only=[1])
    assert rc == ABORTED and "rank 1 of 2: a message to this rank was left unreceived at MPI_Finalize" in se, (rc, se)
    (rc, so, se), = run_rank_program(rank_program, tmp_path / "outside", 4, lambda k: ("outside", 4, 4), only=[2])
    assert rc == ABORTED and "rank 2 of 4: a message to or from a rank outside the grid" in se, (rc, se)
    for size, rank, words in ((3, 0, "CRD_REF_MPI_SIZE is not 1, 2 or 4"), (2, 2, "CRD_REF_MPI_RANK is not a rank of CRD_REF_MPI_SIZE")):
        (rc, so, se), = run_rank_program(rank_program, tmp_path / "env", size, lambda k: ("exchange", 4, 4), only=[rank])
        assert rc == ABORTED and words in se, (rc, se)
