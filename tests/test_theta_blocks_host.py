"""Which grids can see a mistake in the theta-blocks' ghost-column rule: an index-only model of the tile loaders, on the CPU.

A theta-block (SlabDesc::wrap_x == 0) takes the neighbour west of its first column and east of its last one from the strips
gw[j] / ge[j]; crd_rk4_stage_kernel and crd_rhs_aos_kernel (crd_kernels.hip) decide that per 64-column tile:

    iw = (i0 == 0) ? nx - 1 : i0 - 1;  last_col = tx == 63 || i == nx - 1;  ie = (i == nx - 1) ? 0 : i + 1;
    tile[..][0]      = (i0 == 0 && !wrap_x)     ? gw[j] : row[iw];       (lane tx == 0)
    tile[..][tx + 2] = (i == nx - 1 && !wrap_x) ? ge[j] : row[ie];       (lanes with last_col)

supplied_columns() restates this with global column numbers instead of values, and four mutants of it are the slips the rule
invites.  The two per-tile ones -- gw at EVERY tile's first column, ge at EVERY tile's last column -- need a column that starts a
tile without starting the block, or ends a tile without ending the block: a block of 65 columns or more.  No cut of the golden
grids (48, 67 and 32 columns) has one, which is why tests/test_gpu_theta_blocks.py runs the table below.
"""
import numpy as np
import pytest

import crdmodel_amd as crd

TILE = 64

# (nx, d0, d1, ny), the theta widths and phi heights of the cut, and what the entry meets
SHAPES = [
    ((5, 2, 2, 17), (2, 3), (8, 9)),  # the smallest legal block: lane 1 is last_col, no lane is first and last column at once
    ((9, 4, 1, 8), (2, 2, 2, 3), (8,)),  # four blocks, phi wraps inside each (wrap = 1, wrap_x = 0)
    ((127, 2, 3, 26), (63, 64), (8, 9, 9)),  # one tile, one column short and just full
    ((129, 2, 2, 34), (64, 65), (17, 17)),  # a second tile of one column; a second tile row of one row
    ((193, 3, 1, 33), (64, 64, 65), (33,)),  # d0 = 3: the west and the east neighbour are different blocks
    ((257, 2, 2, 40), (128, 129), (20, 20)),  # two full tiles; a third of one column
    ((260, 2, 1, 24), (130, 130), (24,)),  # an interior tile that takes neither branch, a last tile of 2 columns
    ((391, 3, 2, 35), (130, 130, 131), (17, 18)),  # the same, ragged in both directions
    ((258, 4, 3, 50), (64, 65, 64, 65), (16, 17, 17)),  # twelve contexts, alternating widths
]
GOLDEN_CUTS = [(48, 2), (48, 4), (67, 2), (67, 3), (32, 2), (32, 4)]
MUTANTS = ["gw-at-every-tile", "ge-at-every-tile", "wrap-inside-the-block", "strips-swapped"]


def theta_blocks(nx, d0):
    """[(is, ie)] of the d0 theta-blocks of a grid nx wide, from the library's own split rule."""
    return [crd.block_extents(nx, 8, c0, d0, 0, 1)[:2] for c0 in range(d0)]


def supplied_columns(nx, is_, ie_, mutant=None):
    """(W, E): the global column whose value the tile loader hands column is_ + i of the block [is_, ie_] as its west / east
    neighbour.  Inside a tile the neighbours are the tile's own columns (tile[..][tx] and tile[..][tx + 2] are lanes tx - 1 and
    tx + 1); lane 0 and the last_col lane follow the two lines of the module docstring."""
    n = ie_ - is_ + 1  # the block's own nx
    gw, ge = (is_ - 1) % nx, (ie_ + 1) % nx  # what exchange_block_input puts into the strips
    if mutant == "strips-swapped":
        gw, ge = ge, gw
    wrap_x = 1 if mutant == "wrap-inside-the-block" else 0
    W, E = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for i in range(n):
        tx = i % TILE
        i0 = i - tx
        iw = n - 1 if i0 == 0 else i0 - 1
        last_col = tx == TILE - 1 or i == n - 1
        ie = 0 if i == n - 1 else i + 1
        if tx == 0:
            first = True if mutant == "gw-at-every-tile" else i0 == 0
            W[i] = gw if first and not wrap_x else is_ + iw
        else:
            W[i] = is_ + i - 1
        if last_col:
            last = True if mutant == "ge-at-every-tile" else i == n - 1
            E[i] = ge if last and not wrap_x else is_ + ie
        else:
            E[i] = is_ + i + 1
    return W, E


def right(nx, is_, ie_, mutant=None):
    g = np.arange(is_, ie_ + 1)
    W, E = supplied_columns(nx, is_, ie_, mutant)
    return np.array_equal(W, (g - 1) % nx) and np.array_equal(E, (g + 1) % nx)


def test_the_table_holds_the_widths_and_heights_it_claims():
    for (nx, d0, d1, ny), widths, heights in SHAPES:
        assert tuple(ie - is_ + 1 for is_, ie in theta_blocks(nx, d0)) == widths, (nx, d0)
        assert tuple(crd.block_extents(nx, ny, 0, d0, c1, d1)[3] - crd.block_extents(nx, ny, 0, d0, c1, d1)[2] + 1 for c1 in range(d1)) == heights, (ny, d1)
        assert sum(widths) == nx and sum(heights) == ny and min(widths) >= 2 and min(heights) >= 8  # crd_create_block's limits
    every = [w for _, widths, _ in SHAPES for w in widths]
    assert {2, 3, 63, 64, 65, 128, 129, 130, 131} == set(every)
    # every way a block can end: one tile short and full, a tile of one and of two columns behind one and behind two full ones
    assert {w % TILE for w in every if w > TILE} == {0, 1, 2, 3}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d/%d" % s[0][:2])
def test_the_rule_supplies_the_neighbours_of_the_whole_grid(shape):
    nx, d0 = shape[0][:2]
    for is_, ie in theta_blocks(nx, d0):
        assert right(nx, is_, ie), (nx, d0, is_, ie)


def test_the_rule_on_one_block_is_the_plain_wrap():
    """d0 = 1 is wrap_x = 1 in the library: the same lines then wrap inside the row (what the 'wrap inside' mutant does to a block)."""
    for nx in (2, 63, 64, 65, 130):
        assert right(nx, 0, nx - 1, "wrap-inside-the-block")


def test_per_tile_slips_show_from_65_columns_on():
    for mutant in MUTANTS[:2]:
        for nx, d0 in GOLDEN_CUTS:  # what the suite ran before: no block sees either
            for is_, ie in theta_blocks(nx, d0):
                assert right(nx, is_, ie, mutant), (mutant, nx, d0)
        for n in range(2, 3 * TILE + 3):  # a block of n columns in a grid cut in two: seen exactly from 65 on
            assert right(2 * n, 0, n - 1, mutant) == (n <= TILE) and right(2 * n, n, 2 * n - 1, mutant) == (n <= TILE), (mutant, n)
        seen_by = []
        for (nx, d0, _, _), widths, _ in SHAPES:
            seen = [not right(nx, is_, ie, mutant) for is_, ie in theta_blocks(nx, d0)]
            assert seen == [w > TILE for w in widths], (mutant, nx, d0)  # block by block
            if any(seen):
                seen_by.append((nx, d0))
        assert seen_by == [(129, 2), (193, 3), (257, 2), (260, 2), (391, 3), (258, 4)], mutant


def test_whole_strip_slips_show_at_every_entry_and_every_golden_cut():
    """Wrapping inside the block and swapping the strips go wrong at the block's first and last column, whatever its width (a
    theta-block is never the whole row, and with two blocks the ONE neighbour block still supplies two different columns)."""
    for mutant in MUTANTS[2:]:
        for nx, d0 in [s[0][:2] for s in SHAPES] + GOLDEN_CUTS:
            for is_, ie in theta_blocks(nx, d0):
                assert not right(nx, is_, ie, mutant), (mutant, nx, d0)
                g = np.arange(is_, ie + 1)
                W, E = supplied_columns(nx, is_, ie, mutant)  # ... and nowhere else
                assert np.array_equal(W[1:], g[1:] - 1) and np.array_equal(E[:-1], g[:-1] + 1) and W[0] != (is_ - 1) % nx and E[-1] != (ie + 1) % nx
