// The launch planner of madm_conv2d_fwd (conv_plan.hip: pure host code) and what the launcher in igemm.hip shares with it:
// the tile table, the request under decision, and the LDS bound of the split-K + GroupNorm reduction.
#pragma once
#include "igemm_common.hpp"

// The tile codes of madm_conv2d_plan.tile, the tuned tables and madm_debug_set_conv_tile; the names are bench.py's kernel classes.
// IGEMM = register-staged implicit GEMM, `slots` deep (6: for latency-bound small-M GEMMs streaming cold weights); GLDS = fed by
// LDS-DMA through a ring of `slots` stages (+ the 3 KB constant stash of every instantiation: 11 and 17 = 51 KB, three blocks per
// CU; 16 = 35 KB, four, whose prologues and epilogues cover each other on short-K layers; 14 / 15 = 99 / 67 KB, 8 KB of operands
// per MFLOP instead of 11 (128x64) / 31 (64x64): few fat workgroups for launches whose neighbours are other streams' kernels);
// HALO / HALO_DMA = 3x3 conv on 8 x 16-pixel halo patches, weights through registers / LDS-DMA; H16 = 16 x 16-pixel patches, all
// by LDS-DMA, folds a 2x upsample (maps >= 16 x 16); APANEL = A-stationary linear layer (BM / BN only feed the split-K heuristic).
// X(code, BM, BN, family, slots, name), in code order: g_tiles below AND the kernel instantiations launch() in igemm.hip
// dispatches to are both expanded from this one list.
#define MADM_CONV_TILES(X)                                \
    X(1, 128, 128, IGEMM, 2, "igemm_128x128")             \
    X(2, 128, 64, IGEMM, 3, "igemm_128x64")               \
    X(3, 64, 64, IGEMM, 4, "igemm_64x64")                 \
    X(4, 128, 128, HALO, 0, "conv3x3_halo_x128")          \
    X(5, 128, 64, HALO, 0, "conv3x3_halo_x64")            \
    X(6, 64, 64, IGEMM, 8, "igemm_64x64d")                \
    X(7, 64, 64, GLDS, 4, "igemm_glds_64x64")             \
    X(8, 128, 64, GLDS, 3, "igemm_glds_128x64")           \
    X(9, 128, 128, HALO_DMA, 0, "conv3x3_halo_dma_x128")  \
    X(10, 128, 64, HALO_DMA, 0, "conv3x3_halo_dma_x64")   \
    X(11, 64, 64, GLDS, 3, "igemm_glds_64x64s")           \
    X(12, 256, 128, H16, 0, "conv3x3_h16_x128")           \
    X(13, 64, 64, APANEL, 0, "igemm_apanel")              \
    X(14, 128, 128, GLDS, 3, "igemm_glds_128x128")        \
    X(15, 128, 128, GLDS, 2, "igemm_glds_128x128d")       \
    X(16, 64, 64, GLDS, 2, "igemm_glds_64x64d")           \
    X(17, 128, 64, GLDS, 2, "igemm_glds_128x64d")

namespace conv_plan {

enum TileFamily { IGEMM, GLDS, HALO, HALO_DMA, H16, APANEL };
struct Tile { int code, bm, bn; TileFamily family; int slots; const char* name; };
#define MADM_TILE_ROW(code, bm, bn, family, slots, name) {code, bm, bn, family, slots, name},
constexpr Tile g_tiles[] = {MADM_CONV_TILES(MADM_TILE_ROW)};
#undef MADM_TILE_ROW
constexpr int N_TILES = sizeof g_tiles / sizeof g_tiles[0];
inline const Tile* tile_info(int t) { return t >= 1 && t <= N_TILES && g_tiles[t - 1].code == t ? &g_tiles[t - 1] : nullptr; }
inline bool is_igemm_tile(int t) { const Tile* i = tile_info(t); return i && (i->family == IGEMM || i->family == GLDS); }
inline bool is_halo_tile(int t) { const Tile* i = tile_info(t); return i && i->family >= HALO && i->family <= H16; }

// LDS of one (image, group) workgroup of splitk_groupnorm_kernel (igemm.hip), and the most it may ask for
constexpr size_t PGN_MAX_LDS = 96 * 1024;
inline size_t post_gn_lds(int HW, int N, int G) { return (size_t)HW * (size_t)(N / G) * sizeof(float); }

struct Tuned;   // one row of the tuned tables (conv_plan.hip)

// One conv2d request while it is being decided: the arguments as they stand at this stage of the decision, the GEMM they
// describe, and the two process-wide knobs, read ONCE -- every tile / split-K question of one launch is answered from here.
struct Request {
    const madm_conv2d_args* a;
    int M, K;                     // B OH OW, KH KW (C1 + C2)
    int tile_override, profile;   // madm_debug_set_conv_tile, madm_set_tuning_profile
    explicit Request(const madm_conv2d_args* args);
    int k_steps() const { return K / (8 * madm_epc(a->dtype)); }
    int channel_chunks() const { return (a->C1 + a->C2) / (8 * madm_epc(a->dtype)); }
    // the table row of this shape under `variant`: run-time rows, then the latency rows under profile 1, then the throughput table
    const Tuned* row(int variant) const;
};

// what madm_conv2d_fwd asks the planner (conv_plan.hip)
bool halo_eligible(const madm_conv2d_args* a);
void resolve(const Request& r, madm_conv2d_plan& pl);
bool post_gn_fits(const madm_conv2d_args* a, int splitk_eff);
int fill_params(const Request& r, IgemmP& p);   // checks the arguments; everything of IgemmP but splitk / tilesN / the fused GroupNorm
inline size_t splitk_workspace_bytes(int sk, const Request& r) { return sk > 1 ? (size_t)sk * (size_t)r.M * (size_t)r.a->N * sizeof(float) : 0; }

}  // namespace conv_plan
