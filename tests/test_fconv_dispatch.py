"""Characterisation of the fconv dispatch (raft_amd/ops/csrc/fconv_dispatch.h).

The header is plain C++, so a tiny driver built with the host compiler
prints the pick (kernel kind, template arguments, launch grid) for a list
of (shape, alltaps, mtiles, knobs). tests/golden/fconv_dispatch.txt holds
the expected picks; they were recorded from the macro cascade this function
replaced (its launcher compiled host-only with stub kernels that print
their template arguments, one process per RAFT_AMD_* setting), not from
fconv_pick itself. Columns: knobs | label | B H W N C1 in1_stride in1_off
C2 has_in2 kh kw stride mode n_off out_cstride alltaps mtiles | pick | grid.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft_amd", "ops", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fconv_dispatch.txt")
KNOBS = ("BIG_MIN", "TILE2D", "TILE11", "PIPE", "PIPE_BIG", "STEM", "TINYN2")

DRIVER = r"""
#include <cstdio>
#include "fconv_dispatch.h"
int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        FconvKnobs k;
        FconvShape s;
        int has2, at, mt;
        if (sscanf(line, "%lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d "
                   "%d %d %d %d %d %d %d %d", &k.big_min, &k.tile2d,
                   &k.tile11, &k.pipe, &k.pipe_big, &k.stem, &k.tinyn2,
                   &s.B, &s.H, &s.W, &s.N, &s.C1, &s.in1_stride, &s.in1_off,
                   &s.C2, &has2, &s.kh, &s.kw, &s.stride, &s.mode, &s.n_off,
                   &s.out_cstride, &at, &mt) != 24)
            return 2;
        s.has_in2 = has2 != 0;
        const FconvPick p = fconv_pick(s, at, mt, k);
        unsigned g[3];
        switch (p.kind) {
        case FCONV_NONE: printf("none\n"); break;
        case FCONV_STEM:
            printf("stem | %d %d %d\n", (s.N + 31) / 32,
                   s.H * ((s.W + 31) / 32), s.B);
            break;
        case FCONV_TINYN:
            printf("tinyn | %lld 1 1\n",
                   ((long long)s.B * s.H * s.W + 3) / 4);
            break;
        case FCONV_TINYN2:
            printf("tinyn2 | %d 1 %d\n", s.H * ((s.W + 7) / 8), s.B);
            break;
        case FCONV_GENERIC:
            fconv_generic_grid(p, s, g);
            printf("generic %d %d %d %d %d %d %d %d %d | %u %u %u\n", p.KH,
                   p.KW, p.MI, p.NJ, p.AT, p.MT, p.S, p.TH, p.PIPE, g[0],
                   g[1], g[2]);
            break;
        }
    }
    return 0;
}
"""


def _golden():
    rows = []
    with open(GOLDEN) as f:
        for line in f:
            knobs, label, case, want = \
                [c.strip() for c in line.rstrip("\n").split("|", 3)]
            rows.append((knobs, label, case, " ".join(want.split())))
    return rows


def _knob_values(text):
    vals = dict(BIG_MIN=512, TILE2D=7, TILE11=1, PIPE=1, PIPE_BIG=1, STEM=1,
                TINYN2=0)
    if text != "default":
        for kv in text.split():
            k, v = kv.split("=")
            assert k in vals, k
            vals[k] = int(v)
    return " ".join(str(vals[k]) for k in KNOBS)


@pytest.fixture(scope="module")
def picks(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)),
               None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("fconv_dispatch")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True)
    rows = _golden()
    inp = "".join(f"{_knob_values(k)} {case}\n" for k, _, case, _ in rows)
    out = subprocess.run([str(exe)], input=inp, text=True,
                         capture_output=True, check=True).stdout
    got = [" ".join(o.split()) for o in out.splitlines()]
    assert len(got) == len(rows)
    return {(k, lab): (g, want) for (k, lab, _, want), g in zip(rows, got)}


def test_dispatch_matches_recorded_cascade(picks):
    bad = [f"{k} | {lab}: got '{g}', recorded '{w}'"
           for (k, lab), (g, w) in picks.items() if g != w]
    assert not bad, "\n".join(bad)


def test_golden_covers_the_switches():
    rows = _golden()
    assert len({(k, lab) for k, lab, _, _ in rows}) == len(rows)
    knobs = {k for k, _, _, _ in rows}
    for t in (0, 1, 2, 4, 5, 6, 8, 9):
        assert f"TILE2D={t}" in knobs
    for k in ("default", "TILE11=0", "PIPE=0", "PIPE_BIG=0", "STEM=0",
              "BIG_MIN=1", "TILE2D=0 TILE11=0"):
        assert k in knobs
    labels = {lab for k, lab, _, _ in rows if k == "TILE2D=0 TILE11=0"}
    for at in (-1, 0, 1):
        for mt in (-2, 1, 2, 4):
            assert f"cv_3x3@55x128 at={at} mt={mt}" in labels


@pytest.mark.parametrize("label,want", [
    # default knobs, non-big loop shapes: <KH,KW,MI,NJ,AT,MT,S,TH,PIPE>
    ("convc1_1x1@55x128", "generic 1 1 1 1 1 1 1 4 0"),
    ("zr1_1x5@55x128", "generic 1 5 1 1 1 2 1 4 1"),
    ("convc2_3x3@55x128", "generic 3 3 1 1 1 2 1 4 1"),
    ("zr2_5x1@55x128", "generic 5 1 1 1 1 2 1 4 1"),
    # 1080p/8: the big 64x128 tile, never all-taps, pipelined
    ("zr1_1x5@135x240", "generic 1 5 2 4 0 1 1 1 1"),
    ("heads_3x3@135x240", "generic 3 3 2 4 0 1 1 1 1"),
    # N < 128 never takes the big tile
    ("cv_3x3@135x240", "generic 3 3 1 1 1 2 1 4 1"),
    ("fh2_3x3@55x128", "tinyn"),
    ("s2_stem@220x512", "stem"),
    ("s2_5x5_unsupported@110x256", "none"),
])
def test_default_picks(picks, label, want):
    got, _ = picks[("default", label)]
    assert got.split(" |")[0] == want
