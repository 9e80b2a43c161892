// Geometry of the fused correlation lookup -> pointwise conv kernel
// (corr_lookup_conv1x1_k in corr_nhwc.hip) as a pure host function.
//
// No HIP includes: like fconv_dispatch.h this compiles with any host C++
// compiler, so which shapes the kernel serves, its tile, grid and LDS
// size can be characterised on a machine without a GPU
// (tests/test_lookup_conv_geom.py).
//
// One block owns BM consecutive positions (of the flat B*H*W list — a 1x1
// conv needs no spatial tile) and ALL N output channels of them: its
// threads compute the BM x C lookup taps once into an LDS tile of rows of
// Kp = kchunks*32 bf16 (zero tail) plus an 8-element pad, then its `waves`
// waves split the N/16 output-channel tiles of the GEMM among them.
#pragma once

#include <cstdlib>

// row pad (elements): rows of 2*(Kp+8) bytes put the 16 rows of an A
// fragment on 16 distinct 16-byte LDS slots for every Kp multiple of 32
#define LCONV_ROW_PAD 8
#define LCONV_MAX_CS 512      // padded-K cap (LDS tile <= 33 KB at BM=32)
#define LCONV_LDS_PER_CU (160 * 1024)
#define LCONV_WAVES_PER_CU 32

struct LookupConvGeom {
    int ok;             // 0: the shape is not served (use the unfused pair)
    int BM;             // positions per block (16 or 32)
    int waves;          // waves per block (4, 8 or 16) splitting N
    int kchunks;        // 32-wide k-chunks covering Cs
    int row_elems;      // LDS row length in bf16 elements (Kp + pad)
    unsigned grid;      // blocks
    unsigned block;     // threads per block
    int lds_bytes;      // dynamic LDS per block
    int blocks_per_cu;  // co-resident blocks the wave and LDS limits allow
};

// RAFT_AMD_LCONV_TILE: tile variant as BM*100 + waves (1604, 1608, 1616,
// 3204, 3208, 3216); anything else = the default. Read once per process by the
// launcher.
inline int lookup_conv_tile_from_env() {
    const char* e = std::getenv("RAFT_AMD_LCONV_TILE");
    return e ? std::atoi(e) : 0;
}

// positions = B*H*W; C = levels*(2r+1)^2 real taps; Cs = the weights'
// padded input-channel count (zero columns past C); N output channels.
inline LookupConvGeom lookup_conv_geom(long long positions, int C, int Cs,
                                       int N, int tile) {
    LookupConvGeom g{};
    if (positions <= 0 || C <= 0 || Cs < C || Cs % 8 != 0 ||
        Cs > LCONV_MAX_CS || N < 16 || N > 256 || N % 16 != 0)
        return g;
    int bm = 32, waves = 16;                    // default: measured
    switch (tile) {
    case 1604: bm = 16; waves = 4; break;
    case 1608: bm = 16; waves = 8; break;
    case 1616: bm = 16; waves = 16; break;
    case 3204: bm = 32; waves = 4; break;
    case 3208: bm = 32; waves = 8; break;
    case 3216: bm = 32; waves = 16; break;
    default: break;
    }
    const long long blocks = (positions + bm - 1) / bm;
    if (blocks > 0x7fffffffLL) return g;
    g.ok = 1;
    g.BM = bm;
    g.waves = waves;
    g.kchunks = (Cs + 31) / 32;
    g.row_elems = g.kchunks * 32 + LCONV_ROW_PAD;
    g.grid = (unsigned)blocks;
    g.block = (unsigned)(waves * 64);
    g.lds_bytes = bm * g.row_elems * 2;
    const int by_waves = LCONV_WAVES_PER_CU / waves;
    const int by_lds = LCONV_LDS_PER_CU / g.lds_bytes;
    g.blocks_per_cu = by_waves < by_lds ? by_waves : by_lds;
    return g;
}
