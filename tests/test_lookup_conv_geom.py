"""Geometry of the fused lookup -> conv1x1 kernel
(raft_amd/ops/csrc/lookup_conv_geom.h), characterised on the CPU.

The header is plain C++ (as fconv_dispatch.h): a tiny driver built with
the host compiler prints lookup_conv_geom() for a list of (positions, C,
Cs, N, tile). Checked here: which shapes are served, that the blocks of a
grid cover every position exactly once, and that the LDS of the blocks the
geometry claims to co-schedule on a CU fits its 160 KiB.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft_amd", "ops", "csrc")

DRIVER = r"""
#include <cstdio>
#include "lookup_conv_geom.h"
int main() {
    long long p;
    int c, cs, n, tile;
    while (scanf("%lld %d %d %d %d", &p, &c, &cs, &n, &tile) == 5) {
        const LookupConvGeom g = lookup_conv_geom(p, c, cs, n, tile);
        printf("%d %d %d %d %d %u %u %d %d\n", g.ok, g.BM, g.waves,
               g.kchunks, g.row_elems, g.grid, g.block, g.lds_bytes,
               g.blocks_per_cu);
    }
    return 0;
}
"""

TILES = (0, 1604, 1608, 1616, 3204, 3208, 3216)
# positions: the two GPU test shapes (B=2), the headline 55x128, 1080p
# 135x240, and the same two at batch 2 (bidirectional)
POSITIONS = (2 * 16 * 24, 2 * 9 * 17, 55 * 128, 135 * 240, 2 * 55 * 128,
             2 * 135 * 240)
# (C, Cs, N): raft-things and raft-small
MODELS = ((324, 328, 256), (196, 200, 96))


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)),
               None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("lookup_conv_geom")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)

    def run(rows):
        inp = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
        out = subprocess.run([str(exe)], input=inp, text=True,
                             capture_output=True, check=True).stdout
        keys = ("ok", "BM", "waves", "kchunks", "row_elems", "grid", "block",
                "lds_bytes", "blocks_per_cu")
        got = [dict(zip(keys, map(int, line.split())))
               for line in out.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def test_served_shapes(geom):
    rows = [(7040, 324, 328, 256, 0), (7040, 196, 200, 96, 0),
            (7040, 324, 328, 16, 0),
            (7040, 324, 328, 100, 0),     # N no multiple of 16
            (7040, 324, 328, 272, 0),     # N > 256
            (7040, 324, 324, 256, 0),     # Cs no multiple of 8
            (7040, 324, 320, 256, 0),     # Cs < C
            (7040, 600, 600, 256, 0),     # Cs over the LDS cap
            (0, 324, 328, 256, 0)]
    ok = [g["ok"] for g in geom(rows)]
    assert ok == [1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_default_tile_is_a_named_variant(geom):
    d, = geom([(7040, 324, 328, 256, 0)])
    named = geom([(7040, 324, 328, 256, t) for t in TILES[1:]])
    assert d in named
    # an unknown knob value is the default
    assert geom([(7040, 324, 328, 256, 77)])[0] == d


@pytest.mark.parametrize("tile", TILES)
def test_grid_covers_every_position_once(geom, tile):
    rows = [(p, c, cs, n, tile) for p in POSITIONS for c, cs, n in MODELS]
    for (p, c, cs, n, _), g in zip(rows, geom(rows)):
        assert g["ok"] == 1
        assert g["BM"] in (16, 32) and g["waves"] in (4, 8, 16)
        if tile:
            assert g["BM"] * 100 + g["waves"] == tile
        assert g["block"] == 64 * g["waves"]
        # block i owns positions [i*BM, min((i+1)*BM, p)): a partition
        covered = 0
        for i in range(g["grid"]):
            lo, hi = i * g["BM"], min((i + 1) * g["BM"], p)
            assert lo == covered and hi > lo
            covered = hi
        assert covered == p
        # the N/16 channel tiles split over the waves, at most 16/waves each
        per_wave = 16 // g["waves"]
        assert per_wave * g["waves"] * 16 >= n
        # k-chunks cover the padded K; rows hold them plus the pad and stay
        # 16-byte aligned
        assert g["kchunks"] * 32 >= cs > (g["kchunks"] - 1) * 32
        assert g["row_elems"] == g["kchunks"] * 32 + 8
        assert g["row_elems"] * 2 % 16 == 0
        assert g["lds_bytes"] == g["BM"] * g["row_elems"] * 2


@pytest.mark.parametrize("tile", TILES)
def test_lds_within_the_cu(geom, tile):
    rows = [(7040, c, cs, n, tile) for c, cs, n in MODELS]
    rows.append((7040, 512, 512, 256, tile))          # the largest served K
    for g in geom(rows):
        assert g["ok"] == 1
        assert g["lds_bytes"] <= 64 * 1024            # one block's limit
        assert 1 <= g["blocks_per_cu"] <= 32 // g["waves"]
        assert g["lds_bytes"] * g["blocks_per_cu"] <= 160 * 1024
