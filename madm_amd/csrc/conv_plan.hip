// Which kernel a conv2d / linear launch runs on: tile code, split-K and the fusions it can take (madm_conv2d_make_plan and the
// plan madm_conv2d_fwd resolves for itself), from the tuned tables and the heuristics behind them.  Pure host code: the kernels and
// their launcher are in igemm.hip, the tile table and the interface between the two in conv_plan.hpp.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv_plan.hpp"

namespace conv_plan {

// Launch configurations measured on MI355X by tools/tune_insitu.py for the layer shapes of the SD-v1-4
// feature extractor at bs=2, 512x512 (any other shape falls back to the heuristics below).
// variant: 0 = plain, 1 = GroupNorm fused into the halo load, 2 = nearest-2x upsample gather, 3 = stride 2 (a downsample
// conv shares M, N, K with a stride-1 conv of the next level: 8 x 8 x 1280 of the UNet; without a row of its own it takes
// the plain row)
struct Tuned { int dtype, M, N, K, KH, variant, tile, splitk; };

namespace {

int g_tile_override = 0;  // 0 = tuned table then heuristic; -1 = heuristic only; 1..N_TILES = forced tile code
// tile 13 (igemm_apanel.hip): plain linear layer, one source, whole rows resident: no split-K, no residual / time row /
// fused output statistics (its epilogue touches no global memory but the stores)
inline bool apanel_eligible(const madm_conv2d_args* a) {
    return a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad_t == 0 && a->pad_l == 0 && !a->upsample && a->C2 == 0 &&
           a->OH == a->IH && a->OW == a->IW && a->splitk <= 1 && !a->stats && !a->residual && !a->rowvec && !a->gn_sums1 &&
           igemm_apanel_bm(a->C1, (int)madm_esize(a->dtype)) > 0 &&
           // its stores go through a buffer descriptor with 32-bit offsets (0x80000000 = "drop this lane")
           (size_t)a->B * a->OH * a->OW * (size_t)a->ldo * (a->out_f32 ? 4 : madm_esize(a->dtype)) < 0x80000000ull;
}

inline int variant_of(const madm_conv2d_args* a) { return a->gn_sums1 ? 1 : (a->upsample ? 2 : (a->stride == 2 ? 3 : 0)); }
const Tuned g_tuned[] = {
#include "igemm_tuned.inc"
    {-1, 0, 0, 0, 0, 0, 0, 0}};
// The table above is tuned for THROUGHPUT: rows chosen with three launches of the layer side by side (tools/tune_concurrent.py), the
// neighbours a launch has under the runners of madm_amd/pipeline.py.  A synchronous caller -- the reference's loop calling forward()
// with one batch in flight -- wants the choice that is fastest ALONE on an idle chip: more split-K, the tile that fills 256 CUs by
// itself.  Profile 1 (madm_set_tuning_profile; ops.tuning_profile("latency")) puts these rows in front of the table; a shape without
// one keeps its throughput row.
const Tuned g_tuned_latency[] = {
#include "igemm_tuned_latency.inc"
    {-1, 0, 0, 0, 0, 0, 0, 0}};
std::atomic<int> g_tuning_profile{0};

// Run-time rows in front of the compiled-in table (A/B runs of tools/tune_concurrent.py without a rebuild): the file named
// by MADM_TUNED_FILE holds one "dtype M N K KH variant tile splitk" row per line ('#' starts a comment); read once.
const std::vector<Tuned>& tuned_overrides() {
    static const std::vector<Tuned> rows = [] {
        std::vector<Tuned> v;
        const char* path = getenv("MADM_TUNED_FILE");
        if (!path || !*path) return v;
        FILE* f = fopen(path, "r");
        if (!f) { fprintf(stderr, "madm: MADM_TUNED_FILE=%s cannot be opened\n", path); return v; }
        char line[256];
        while (fgets(line, sizeof line, f)) {
            Tuned t;
            if (line[0] == '#') continue;
            if (sscanf(line, "%d %d %d %d %d %d %d %d", &t.dtype, &t.M, &t.N, &t.K, &t.KH, &t.variant, &t.tile, &t.splitk) != 8)
                continue;
            // a row with an unknown tile code would fall through to the default igemm launch unnoticed: refuse it loudly
            if (!tile_info(t.tile) || t.splitk < 1 || t.variant < 0 || t.variant > 3 || !madm_dtype_ok(t.dtype)) {
                fprintf(stderr, "madm: MADM_TUNED_FILE=%s: row ignored (tile 1..%d, splitk >= 1, variant 0..3): %s", path, N_TILES, line);
                continue;
            }
            v.push_back(t);
        }
        fclose(f);
        return v;
    }();
    return rows;
}

int heuristic_tile(int M, int N, int K) {
    auto tiles = [&](int bm, int bn) { return (long long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    // shapes without a tuned entry (the segmentation head, the training step's gradients, other batch sizes): the
    // register-staged 128 x 128 tile never wins a tuned entry and loses 25 .. 40 % on the head's M = 524 288 GEMMs
    // (M524288: N256 K1024 851 us vs 612 (tile 8) / 630 (tile 2); N1024 K256 1447 vs 892 (tile 2); MI355X, f16)
    if (M >= 128 && tiles(128, 64) >= 256) return K >= 1024 ? 8 : 2;
    return 3;
}

// narrowest map the halo kernels take: an 8-wide map wastes half of every 8 x 16 patch, but lets the 8 x 8 UNet level fuse
// its GroupNorm
constexpr int HALO_MIN_W = 8;

int pick_tile_raw(const Request& r) {
    const madm_conv2d_args* a = r.a;
    const int forced = r.tile_override;
    const bool halo_ok = halo_eligible(a);
    const int halo_default = (a->N % 128 == 0 || a->N >= 512) ? 4 : 5;
    if (a->gn_sums1) {   // fused GroupNorm exists only in the halo kernels
        if (is_halo_tile(forced)) return forced;
        if (const Tuned* t = r.row(variant_of(a)))
            if (is_halo_tile(t->tile)) return t->tile;
        return halo_default;
    }
    if (is_igemm_tile(forced) || (is_halo_tile(forced) && halo_ok))
        return forced;   // (13 = the A-stationary kernel is handled by pick_tile; ineligible launches fall through)
    if (const Tuned* t = r.row(variant_of(a)))
        if (is_igemm_tile(t->tile) || halo_ok) return t->tile;
    if (halo_ok && r.M >= 2048) return halo_default;
    return heuristic_tile(r.M, a->N, r.K);
}

// the 16 x 16-patch kernel pays where it fills the chip: at least ~0.75 rounds of its 256-pixel x 128-channel blocks
// (measured against tile 9 on MI355X, bf16 / f16: +12 .. 23 % on the 512^2 .. 128^2 maps of the VAE, 0.6 x on an 8192-pixel map)
bool h16_pays(const madm_conv2d_args* a) {
    if (a->OH < 16 || a->OW < 16 || a->N < 128) return false;
    const long long blocks = (long long)a->B * ((a->OH + 15) / 16) * ((a->OW + 15) / 16) * ((a->N + 127) / 128);
    return blocks >= 384;
}

// nearest-2x upsample + 3x3 conv (Upsample2D of the VAE decoder / UNet): only the 16 x 16-patch kernel folds the
// upsample into its halo gather (igemm 128x64 on the 256-channel 512 x 512 layer: 456 us, this kernel: see DESIGN.md)
bool h16_upsample_eligible(const madm_conv2d_args* a) {
    return a->KH == 3 && a->KW == 3 && a->stride == 1 && a->pad_t == 1 && a->pad_l == 1 && a->upsample &&
           a->OH == 2 * a->IH && a->OW == 2 * a->IW && !a->gn_sums1 && a->epilogue != MADM_EPI_GEGLU && a->OH >= 16 &&
           a->OW >= 16;
}

int pick_tile(const Request& r) {
    const madm_conv2d_args* a = r.a;
    if (apanel_eligible(a)) {   // (K = C1, KH = 1, variant 0)
        if (r.tile_override == 13) return 13;
        if (const Tuned* t = r.row(0))
            if (t->tile == 13) return 13;
    }
    if (h16_upsample_eligible(a)) {
        // a table row decides (variant 2; the side-by-side tuner put the UNet's upsample convs here although their grids
        // are far below a round of workgroups), h16_pays() where there is none; no row is looked up under a tile override
        const Tuned* t = r.row(2);
        if (r.tile_override == 12 || (t ? t->tile == 12 : (r.tile_override == 0 && h16_pays(a)))) return 12;
    }
    const int t = pick_tile_raw(r);
    if (t == 12 && (a->OH < 16 || a->OW < 16)) return 9;   // the 16 x 16-patch kernel needs a map of at least one patch
    if ((t == 4 || t == 9) && r.tile_override == 0 && h16_pays(a)) return 12;
    return t;
}

// split-K for the 256 CUs of MI355X where the request leaves it to the library: the row's if its tile is the one chosen, else about two rounds
int suggest_splitk(const Request& r) {
    const int chosen = pick_tile(r), nk = r.k_steps();
    if (const Tuned* t = r.row(variant_of(r.a)))
        if (t->tile == chosen) return t->splitk;
    const Tile* ti = tile_info(chosen);
    const long long tiles = (long long)((r.M + ti->bm - 1) / ti->bm) * ((r.a->N + ti->bn - 1) / ti->bn);
    if (tiles >= 192 || nk < 8) return 1;
    return (int)std::max(1LL, std::min({(512 + tiles - 1) / tiles, nk / 4LL, 32LL}));
}

}  // namespace

Request::Request(const madm_conv2d_args* args)
    : a(args), M(args->B * args->OH * args->OW), K(args->KH * args->KW * (args->C1 + args->C2)),
      tile_override(g_tile_override), profile(g_tuning_profile.load(std::memory_order_relaxed)) {}

const Tuned* Request::row(int variant) const {
    if (tile_override != 0) return nullptr;
    const int dt = a->dtype == MADM_F16 ? MADM_BF16 : a->dtype;   // same kernels, same instruction rate: the bf16 table serves both
    auto hit = [&](const Tuned& t) { return t.dtype == dt && t.M == M && t.N == a->N && t.K == K && t.KH == a->KH && t.variant == variant; };
    for (const Tuned& t : tuned_overrides())
        if (hit(t)) return &t;
    for (const Tuned* t = g_tuned_latency; profile == 1 && t->dtype >= 0; ++t)
        if (hit(*t)) return t;
    for (const Tuned* t = g_tuned; t->dtype >= 0; ++t)
        if (hit(*t)) return t;
    return variant == 3 ? row(0) : nullptr;
}

// the LDS halo-tile kernel (conv3x3.hip) handles 3x3 / stride 1 / pad 1 convs on maps of at least one patch
bool halo_eligible(const madm_conv2d_args* a) {
    return a->KH == 3 && a->KW == 3 && a->stride == 1 && a->pad_t == 1 && a->pad_l == 1 && !a->upsample &&
           a->OH == a->IH && a->OW == a->IW && a->OH >= 8 && a->OW >= HALO_MIN_W && a->epilogue != MADM_EPI_GEGLU;
}

// the arguments taken as they stand: the tile madm_conv2d_fwd launches and the split-K its kernels run with (at least one K step
// per slice; the halo kernels split K by whole channel chunks)
void resolve(const Request& r, madm_conv2d_plan& pl) {
    pl.tile = pick_tile(r);
    pl.splitk = r.a->splitk;
    pl.splitk_eff = std::min(pl.splitk, r.k_steps());
    if (is_halo_tile(pl.tile)) pl.splitk_eff = std::min(pl.splitk_eff, r.channel_chunks());
    pl.splitk_eff = std::max(pl.splitk_eff, 1);
    pl.workspace_bytes = splitk_workspace_bytes(pl.splitk, r);
}

// can the split-K reduction of this launch apply the consumer's GroupNorm (pn_groups)?
bool post_gn_fits(const madm_conv2d_args* a, int splitk_eff) {
    if (splitk_eff <= 1 || a->pn_groups <= 0 || a->N <= 0 || a->N % a->pn_groups) return false;
    if (a->epilogue != MADM_EPI_NONE || a->residual || a->stats || a->out_f32 || a->ln_colsum) return false;
    return (a->N / a->pn_groups) % 2 == 0 && post_gn_lds(a->OH * a->OW, a->N, a->pn_groups) <= PGN_MAX_LDS;
}

int fill_params(const Request& r, IgemmP& p) {
    const madm_conv2d_args* a = r.a;
    const int bke = (8 * madm_epc(a->dtype));
    MADM_REQUIRE(a->in1 && a->w && a->out, "conv2d: null tensor pointer");
    MADM_REQUIRE(a->C1 > 0 && a->C1 % bke == 0, "conv2d: C1=%d must be a positive multiple of %d", a->C1, bke);
    MADM_REQUIRE(a->C2 >= 0 && a->C2 % bke == 0, "conv2d: C2=%d must be a multiple of %d", a->C2, bke);
    MADM_REQUIRE(a->C2 == 0 || a->in2, "conv2d: C2>0 needs in2");
    MADM_REQUIRE(a->B > 0 && a->IH > 0 && a->IW > 0 && a->OH > 0 && a->OW > 0, "conv2d: bad dims");
    MADM_REQUIRE(a->KH > 0 && a->KW > 0 && a->stride > 0, "conv2d: bad kernel/stride");
    MADM_REQUIRE(a->N > 0 && a->N % 4 == 0, "conv2d: N=%d must be a positive multiple of 4", a->N);
    MADM_REQUIRE(a->epilogue >= MADM_EPI_NONE && a->epilogue <= MADM_EPI_RELU, "conv2d: bad epilogue");
    MADM_REQUIRE(a->splitk >= 1, "conv2d: splitk must be >= 1");
    const int ocols = (a->epilogue == MADM_EPI_GEGLU) ? a->N / 2 : a->N;
    MADM_REQUIRE(a->ldo >= ocols && a->ldo % 2 == 0, "conv2d: ldo=%d too small/odd for %d columns", a->ldo, ocols);
    MADM_REQUIRE(a->epilogue == MADM_EPI_GEGLU || a->ldo % 4 == 0, "conv2d: ldo must be a multiple of 4");
    MADM_REQUIRE(!a->residual || (a->ldr >= ocols && a->ldr % 2 == 0), "conv2d: bad ldr");
    p.in1 = (const char*)a->in1; p.in2 = (const char*)a->in2; p.w = (const char*)a->w;
    p.bias = a->bias; p.rowvec = a->rowvec; p.residual = (const char*)a->residual;
    p.out = (char*)a->out; p.ws = (float*)a->workspace; p.stats = a->stats;
    p.gn_sums1 = nullptr; p.gn_sums2 = nullptr; p.gn_gamma = nullptr; p.gn_beta = nullptr;
    p.gn_G = 0; p.gn_eps = 0.f; p.gn_magic = 0; p.act = 0;
    p.ln_cs = a->ln_colsum; p.ln_eps = a->ln_eps;
    if (a->ln_colsum) {
        MADM_REQUIRE(a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad_t == 0 && a->pad_l == 0 && !a->upsample &&
                     a->C2 == 0 && a->OH == a->IH && a->OW == a->IW,
                     "conv2d: the folded LayerNorm needs a linear layer / 1x1 conv over ONE source (K = C1)");
        MADM_REQUIRE(!a->gn_sums1 && a->ln_eps > 0.f && a->splitk == 1,
                     "conv2d: folded LayerNorm: no fused GroupNorm, eps > 0, splitk == 1 (every block must see whole rows)");
    }
    MADM_REQUIRE(!a->stats || a->epilogue != MADM_EPI_GEGLU, "conv2d: fused statistics cannot follow GEGLU");
    p.C1 = a->C1; p.C2 = a->C2; p.Ctot = a->C1 + a->C2;
    p.B = a->B; p.IH = a->IH; p.IW = a->IW; p.OH = a->OH; p.OW = a->OW;
    p.KH = a->KH; p.KW = a->KW; p.stride = a->stride; p.pad_t = a->pad_t; p.pad_l = a->pad_l;
    p.upsample = a->upsample ? 1 : 0;
    p.N = a->N; p.K = r.K; p.M = r.M;
    MADM_REQUIRE(!a->rowvec || (a->ldrv >= a->N && a->ldrv % 4 == 0), "conv2d: bad ldrv=%d", a->ldrv);
    p.ldr = a->ldr; p.ldo = a->ldo; p.ldrv = a->ldrv; p.epilogue = a->epilogue;
    p.ldw = a->ldw ? a->ldw : p.K;
    p.out_f32 = a->out_f32 ? 1 : 0;
    MADM_REQUIRE(p.ldw >= p.K && p.ldw % (bke / 8) == 0, "conv2d: bad weight row stride ldw=%d", p.ldw);
    MADM_REQUIRE(!p.out_f32 || (a->epilogue != MADM_EPI_GEGLU && !a->residual), "conv2d: out_f32 cannot follow GEGLU / residual");
    p.ld1 = a->ld1 ? a->ld1 : a->C1;
    p.ld2 = a->ld2 ? a->ld2 : a->C2;
    MADM_REQUIRE(p.ld1 >= a->C1 && p.ld2 >= a->C2 && p.ld1 % (bke / 8) == 0 && p.ld2 % (bke / 8) == 0,
                 "conv2d: bad source row strides ld1=%d ld2=%d", p.ld1, p.ld2);
    {
        const size_t es = madm_esize(a->dtype);
        const size_t px = (size_t)a->B * a->IH * a->IW;
        const size_t b1 = ((px - 1) * p.ld1 + a->C1) * es;
        const size_t b2 = a->C2 ? ((px - 1) * p.ld2 + a->C2) * es : 0;
        const size_t bw = ((size_t)(a->N - 1) * p.ldw + p.K) * es;
        MADM_REQUIRE(b1 < 0x80000000ull && b2 < 0x80000000ull && bw < 0x80000000ull,
                     "conv2d: tensors must stay below 2 GiB (32-bit buffer offsets)");
        p.bytes1 = (unsigned)b1; p.bytes2 = (unsigned)b2; p.bytesw = (unsigned)bw;
    }
    p.nk = r.k_steps();
    MADM_REQUIRE((long long)p.nk * (std::min(a->splitk, p.nk) + 1) < 0x7fffffffLL, "conv2d: K too large for the 32-bit slice arithmetic");
    // Alignment (include/madm_hip.h states it next to every field).  Sources and weights are read in 16-byte chunks (registers or
    // LDS-DMA); bias / rowvec / ln_colsum and the GroupNorm parameters as float4; out and residual in units of 4 elements (2 under
    // GEGLU) -- 8 bytes in the 16-bit modes, where only the 16 x 16-patch kernel's LDS-transposed path moves 16 bytes and looks
    // at the pointers itself (launch_conv3x3_h16); the statistics are f64 atomics.
    {
        auto al = [](const void* q, size_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; };
        const size_t ounit = (a->epilogue == MADM_EPI_GEGLU ? 2 : 4) * (a->out_f32 ? 4 : madm_esize(a->dtype));
        const size_t runit = (a->epilogue == MADM_EPI_GEGLU ? 2 : 4) * madm_esize(a->dtype);
        MADM_REQUIRE(al(a->in1, 16) && al(a->in2, 16) && al(a->w, 16), "conv2d: in1 / in2 / w must be 16-byte aligned");
        MADM_REQUIRE(al(a->bias, 16) && al(a->rowvec, 16) && al(a->ln_colsum, 16) && al(a->gn_gamma, 16) && al(a->gn_beta, 16) &&
                     al(a->pn_gamma, 16) && al(a->pn_beta, 16) && al(a->workspace, 16),
                     "conv2d: bias / rowvec / ln_colsum / gn_* / pn_* parameters and the workspace must be 16-byte aligned");
        MADM_REQUIRE(al(a->stats, 8) && al(a->gn_sums1, 8) && al(a->gn_sums2, 8), "conv2d: f64 statistics must be 8-byte aligned");
        MADM_REQUIRE(al(a->out, ounit), "conv2d: out must be aligned to %zu bytes", ounit);
        MADM_REQUIRE(!a->residual || (al(a->residual, runit) && (a->epilogue == MADM_EPI_GEGLU || a->ldr % 4 == 0)),
                     "conv2d: residual must be aligned to %zu bytes and ldr a multiple of 4 (2 under GEGLU)", runit);
    }
    return MADM_OK;
}

}  // namespace conv_plan

using namespace conv_plan;

extern "C" {

void madm_debug_set_conv_tile(int t) { g_tile_override = t; }

int madm_set_tuning_profile(int profile) {
    MADM_REQUIRE(profile == 0 || profile == 1, "set_tuning_profile: 0 = throughput (side-by-side rows), 1 = latency (lone-launch rows)");
    g_tuning_profile.store(profile, std::memory_order_relaxed);
    return MADM_OK;
}
int madm_get_tuning_profile(void) { return g_tuning_profile.load(std::memory_order_relaxed); }

const char* madm_conv2d_tile_name(int tile) { return tile_info(tile) ? tile_info(tile)->name : nullptr; }

// A caller used to decide in stages, each on what the earlier ones had filled in (apanel_eligible looks at splitk and stats): split-K
// suggested for the tile picked WITHOUT split-K and statistics, the post-GroupNorm asked with the split-K set and still no statistics,
// the launch picked with everything set.  The same stages run here, on one copy of the request and one reading of the process state.
int madm_conv2d_make_plan(const madm_conv2d_args* request, madm_conv2d_plan* plan) {
    MADM_REQUIRE(request != nullptr && plan != nullptr, "conv2d plan: null argument");
    MADM_REQUIRE(madm_dtype_ok(request->dtype), "conv2d plan: bad dtype %d", request->dtype);
    MADM_REQUIRE(request->splitk >= 0, "conv2d plan: splitk must be 0 (the library chooses) or >= 1");
    madm_conv2d_args c = *request;
    const Request r(&c);
    c.stats = nullptr; c.pn_gamma = nullptr;
    if (request->splitk == 0) {
        c.splitk = 1;
        c.splitk = std::max(1, suggest_splitk(r));
    }
    resolve(r, *plan);
    plan->post_gn = post_gn_fits(&c, plan->splitk_eff) ? 1 : 0;
    if (!plan->post_gn && request->stats) {   // the statistics come from the conv's own epilogue
        c.stats = request->stats;
        resolve(r, *plan);
    }
    // a row was FOUND for the shape: the stride-2 -> plain fallback and the upsample lookup count
    plan->tuned_row = ((h16_upsample_eligible(&c) && r.row(2)) || r.row(variant_of(&c))) ? 1 : 0;
    return MADM_OK;
}

int madm_conv2d_can_fuse_groupnorm(const madm_conv2d_args* a) { return a && halo_eligible(a) ? 1 : 0; }

}  // extern "C"
