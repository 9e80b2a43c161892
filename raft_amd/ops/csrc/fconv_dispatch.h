// fconv dispatch: which kernel a conv shape gets, as a pure host function.
//
// No HIP includes: this header compiles with any host C++ compiler, so the
// whole precedence order can be characterised on a machine without a GPU
// (tests/test_fconv_dispatch.py). fconv.hip turns the returned FconvPick
// into a launch through one instantiation table; a pick that names no
// instantiated kernel is a hard error there.
#pragma once

#include <cstdlib>

// RAFT_AMD_* switches steering the pick (documented in ARCHITECTURE.md).
// The launcher reads them once per process.
struct FconvKnobs {
    long long big_min = 512;  // RAFT_AMD_BIG_MIN: 64x128-tiling block count
                              // from which the big tile is used
    int tile2d = 7;           // RAFT_AMD_TILE2D: 2D output tiles (TH > 1)
    int tile11 = 1;           // RAFT_AMD_TILE11: 32x32 instead of 32x64
    int pipe = 1;             // RAFT_AMD_PIPE: register-prefetch k-loop
    int pipe_big = 1;         // RAFT_AMD_PIPE_BIG: ... for the big tile too
    int stem = 1;             // RAFT_AMD_STEM: dedicated 7x7-S2/C8 kernel
    int tinyn2 = 0;           // RAFT_AMD_TINYN2: row-tile-staged N=2 kernel
};

inline FconvKnobs fconv_knobs_from_env() {
    FconvKnobs k;
    if (const char* e = std::getenv("RAFT_AMD_BIG_MIN")) k.big_min = std::atoll(e);
    if (const char* e = std::getenv("RAFT_AMD_TILE2D")) k.tile2d = std::atoi(e);
    if (const char* e = std::getenv("RAFT_AMD_TILE11")) k.tile11 = std::atoi(e);
    if (const char* e = std::getenv("RAFT_AMD_PIPE")) k.pipe = std::atoi(e);
    if (const char* e = std::getenv("RAFT_AMD_PIPE_BIG")) k.pipe_big = std::atoi(e);
    if (const char* e = std::getenv("RAFT_AMD_STEM")) k.stem = std::atoi(e);
    if (const char* e = std::getenv("RAFT_AMD_TINYN2")) k.tinyn2 = std::atoi(e);
    return k;
}

// What the launcher is asked to compute. H, W are OUTPUT dims (stride 2:
// input = 2H x 2W). C2 / has_in2 describe the optional second input.
struct FconvShape {
    int B, H, W, N;
    int C1, in1_stride, in1_off;
    int C2;
    bool has_in2;
    int kh, kw, stride;
    int mode;                 // epilogue (0 = plain)
    int n_off, out_cstride;   // output channel slice
};

enum FconvKind {
    FCONV_NONE = 0,   // unsupported shape: the launcher refuses it
    FCONV_GENERIC,    // fconv_nhwc_bf16_k<KH,KW,MI,NJ,AT,MT,S,TH,PIPE>
    FCONV_STEM,       // fconv_stem_s2_k
    FCONV_TINYN,      // fconv_tinyn_k<2>
    FCONV_TINYN2,     // fconv_tinyn2_k<2>
};

struct FconvPick {
    FconvKind kind;
    // template arguments of the generic kernel (0 for the other kinds)
    int KH, KW, MI, NJ, AT, MT, S, TH, PIPE;
};

// Launch grid of a generic pick: blocks of 32*NJ output channels by a
// position tile of TH rows x (MT*32*MI/TH) columns.
inline void fconv_generic_grid(const FconvPick& p, const FconvShape& sh,
                               unsigned grid[3]) {
    const int bn = 32 * p.NJ;
    const int bx = p.MT * 32 * p.MI / p.TH;
    grid[0] = (unsigned)((sh.N + bn - 1) / bn);
    grid[1] = (unsigned)(((sh.H + p.TH - 1) / p.TH) * ((sh.W + bx - 1) / bx));
    grid[2] = (unsigned)sh.B;
}

// The row-tile-staged N=2 kernel holds its window and all weights in LDS.
inline bool fconv_tinyn2_ok(const FconvKnobs& k, int Cin, int kh, int kw) {
    // measured: dead even with the cell-per-wave kernel on the headline
    // config (9.796 vs 9.799 ms/step) — the shared windows are already
    // L2-resident there. Kept selectable (RAFT_AMD_TINYN2=1) for shapes
    // whose windows spill L2.
    return k.tinyn2 && Cin % 8 == 0 && Cin <= 256 && kh <= 3 && kw <= 3;
}

// alltaps: -1 auto, 0/1 force the all-taps (AT) staging off/on.
// mtiles: >0 = m-tiles per block for the 32x64 tile (1, 2, 4 exist),
// -1 auto (= 1), -2 = force the big (64x128) tile regardless of grid size
// (structure-efficiency probes).
inline FconvPick fconv_pick(const FconvShape& sh, int alltaps, int mtiles,
                            const FconvKnobs& knobs) {
    const int kh = sh.kh, kw = sh.kw;
    const auto generic = [](int KH, int KW, int MI, int NJ, bool AT, int MT,
                            int S, int TH, bool PIPE) {
        return FconvPick{FCONV_GENERIC, KH, KW, MI, NJ, AT, MT, S, TH, PIPE};
    };
    const FconvPick none{FCONV_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    // large tile (64x128) when it still fills the chip, else small tiles:
    // MI355X has 256 CUs / 8 XCDs — batch-1 grids need the small ones.
    // N < 128 leaves half the big tile's 128 output-channel columns idle
    // (measured: encoder N=64 3x3s run 80.7 us big vs ~55 us small even at
    // 3520 blocks) — the big tile requires a full N extent.
    const long long big_blocks = (long long)((sh.N + 127) / 128) * sh.H *
                                 ((sh.W + 63) / 64) * sh.B;
    const bool big = big_blocks >= knobs.big_min && sh.N >= 128;

    // N = 2 (the flow head's final 3x3): one wave per position
    if (sh.N == 2 && sh.mode == 0 && !sh.has_in2 && sh.n_off == 0 &&
        sh.out_cstride == sh.N) {
        FconvPick p = none;
        p.kind = fconv_tinyn2_ok(knobs, sh.C1, kh, kw) ? FCONV_TINYN2
                                                       : FCONV_TINYN;
        return p;
    }

    // stride-2 (encoder) shapes
    if (sh.stride == 2) {
        if (knobs.stem && kh == 7 && kw == 7 && sh.C1 == 8 && sh.C2 == 0 &&
            sh.mode == 0 && sh.n_off == 0 && sh.out_cstride == sh.N &&
            sh.in1_off == 0 && sh.in1_stride == 8 && sh.N <= 128) {
            FconvPick p = none;
            p.kind = FCONV_STEM;
            return p;
        }
        if (kh != kw || (kh != 7 && kh != 3 && kh != 1)) return none;
        return big ? generic(kh, kw, 2, 4, false, 1, 2, 1, false)
                   : generic(kh, kw, 1, 2, false, 1, 2, 1, false);
    }

    const bool k11 = kh == 1 && kw == 1, k33 = kh == 3 && kw == 3;
    const bool k15 = kh == 1 && kw == 5, k51 = kh == 5 && kw == 1;
    if (!k11 && !k33 && !k15 && !k51) return none;

    // big tile: never all-taps (LDS kills occupancy: heads 3x3 N=512
    // 30.2 -> 39.8 us); pipelined since r2 (1080p loop convs dispatch big
    // and ran unpipelined at ~100 us, ~13% MFMA)
    if (big || mtiles == -2)
        return generic(kh, kw, 2, 4, false, 1, 1, 1, knobs.pipe_big != 0);

    // all-taps staging (measured, tools/bench_fconv.py): wins for kh>1 on
    // the small tiles (5x1: 43.6 -> 32.8 us; 3x3 convc2: 35.5 -> 28.4)
    const bool at = (alltaps < 0) ? kh > 1 : (alltaps != 0);
    // PIPE measured: -8..-20% on 3x3/1x5/5x1 q/cv shapes, +3 us on 1x1
    // (short k-loop, extra regs) — so 1x1 stays unpipelined.
    const bool pipe = knobs.pipe != 0 && !k11;
    const int t2 = knobs.tile2d;

    // 2D output tiles (TH rows x 32/TH cols, all-taps, MI = 1): vertical
    // taps share staged row slabs. Measured on the headline config: TH=2
    // 11.98 -> 11.77, TH=4 -> 10.64 ms/step, TH=4 incl. 1x5 -> 10.29 (the
    // 4-row tile wins even where it stages MORE halo, so the lever is
    // occupancy, not just staging ratio), incl. 1x1 -> 10.21, MT2 under
    // TH4+PIPE 9.23 -> 8.98 (B-slice staging was the bound for the zr
    // shapes). RAFT_AMD_TILE2D: 0 = off, 1 = TH2 (KH>1), 2 = TH2 with
    // NJ2/BN64 (worse: LDS-limited occupancy), 4 = TH4 for KH>1, 5 = TH4
    // incl. 1x5, 6 = MT2 under TH4 for KH>1 and 1x5, 7 (default) = 6 plus
    // TH4 for 1x1, 8 = TH8 for 5x1 (parity with TH4), 9 = NJ2 under TH4
    // (16x32 wave tiles, 2x MFMA per barrier; loses: halved grid).
    if (k11 && t2 == 7) return generic(1, 1, 1, 1, true, 1, 1, 4, pipe);
    if (k15) {
        if (t2 == 9) return generic(1, 5, 1, 2, true, 1, 1, 4, pipe);
        if (t2 == 6 || t2 == 7) return generic(1, 5, 1, 1, true, 2, 1, 4, pipe);
        if (t2 == 5) return generic(1, 5, 1, 1, true, 1, 1, 4, pipe);
    }
    if (kh > 1 && t2 && at) {
        if (t2 == 2) return generic(kh, kw, 1, 2, true, 1, 1, 2, pipe);
        if (t2 == 8 && k51) return generic(5, 1, 1, 1, true, 1, 1, 8, pipe);
        if (t2 == 9) return generic(kh, kw, 1, 2, true, 1, 1, 4, pipe);
        if (t2 == 6 || t2 == 7) return generic(kh, kw, 1, 1, true, 2, 1, 4, pipe);
        if (t2 >= 4) return generic(kh, kw, 1, 1, true, 1, 1, 4, pipe);
        return generic(kh, kw, 1, 1, true, 1, 1, 2, pipe);
    }

    // 1D tiles of one output row, unpipelined; all-taps only for kh > 1
    const bool at1 = kh > 1 && at;
    // 32x32 (2x the workgroups of 32x64): measured 12.74 -> 12.54 ms/step
    // on the headline config. 5x1 excluded: vertical taps share no staged
    // rows, so the extra workgroups just duplicate A slabs (39.1 vs 37.7).
    if (knobs.tile11 && !k51)
        return generic(kh, kw, 1, 1, at1, 1, 1, 1, false);
    // 32x64 with MT m-tiles per block. MT>1 was hypothesized to win by
    // amortizing per-block weight staging but MEASURED worse nearly
    // everywhere (grid saturation dominates at batch-1 sizes) — kept
    // selectable for larger-batch shapes.
    const int mt = mtiles >= 4 ? 4 : (mtiles == 2 ? 2 : 1);
    return generic(kh, kw, 1, 2, at1, mt, 1, 1, false);
}
