// render.hip -- liblle_render.so: batched RGB frames of an lle_batch (C ABI: include/lle_render.h).
//
// The renderer of the reference (src/rendering/renderer.rs, sprites.rs) for many environments in one launch.  The library reads a
// batch only through the public ABI of include/lle_hip.h (lle_batch_get_buffer, lle_map_*), so liblle_hip.so keeps its kernels.
//
// Frame of one environment: (32 H + 1) x (32 W + 1) RGB pixels, HWC.  A pixel's colour depends on its cell only (every sprite and
// every static drawing of the reference covers its own 32 x 32 tile), so a frame is
//   grid line (x % 32 == 0 or y % 32 == 0)                      GRID_GREY, drawn last (renderer.rs:106,119-130)
//   otherwise: the cell's static tile (floor / wall / exit / void, renderer.rs:39-73), then the sprites the cell's draw list
//   resolves to for this environment, blended in the reference's order (renderer.rs:75-108):
//     for each entry of World::lasers() on the cell (the outer layer and, when nested, the second one; world.rs:159-172):
//        draw_laser recursing through the wrapped tiles (renderer.rs:187-198): every layer from that one down that is on, then
//        the gem under the stack if it is not collected
//     the gem, again, if it is not collected (renderer.rs:85-92)
//     every agent standing there, in id order (renderer.rs:93-97)
//     the laser source, opaque (renderer.rs:98-105; alpha 255 blends to the sprite's RGB exactly)
// The host turns each map into a per-cell list of draw OPS (static), the kernel resolves the ops of one row of cells per workgroup
// into sprite ids in LDS (dynamic: beams, colours, gems, agents) and then streams the row's 32 pixel lines as 16-byte chunks.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_render.h"
#include "../common/abi_host.hpp"

// Rust does not contract `(1 - a) * bg + a * fg` into an FMA; clang would (host and device): every blend below is
// rounded op by op.
#pragma clang fp contract(off)


namespace lle {

constexpr int TILE = 32;
constexpr int TILE_PX = TILE * TILE;
constexpr int RENDER_THREADS = 256;
constexpr int MAX_CELL_OPS = 10;   // a gem under four beams: 4 + 1 (outer entry) + 3 + 1 (second entry) + 1 (gem loop)
constexpr int MAX_DRAWS = 32;      // resolved sprites of one cell: its ops and up to 16 agents
constexpr uint32_t GRID_GREY = 127u | 127u << 8 | 127u << 16;
constexpr uint32_t BACKGROUND_GREY = 218u | 218u << 8 | 218u << 16;

// op word: bits 30-31 the kind
//   OP_LASER   0-7 colour of the map's source, 8-12 beam word, 13-17 bit, 18 vertical beam
//   OP_GEM     0-5 gem index
//   OP_SOURCE  0-7 colour of the map's source, 8-12 first beam word of the source, 13-14 direction (N E S W)
// cell word: bits 0-1 static tile (floor, wall, exit, void), 2-5 number of ops, 6-31 first op (index into the map's ops)
enum : uint32_t { OP_LASER = 0u, OP_GEM = 1u, OP_SOURCE = 2u };
enum : uint32_t { TILE_FLOOR = 0u, TILE_WALL = 1u, TILE_EXIT = 2u, TILE_VOID = 3u };

struct RenderParams {
    const uint32_t* tables;    // per map: [H*W] cell words, then its ops
    const uint32_t* map_off;   // [n_maps] first word of each map's tables
    const uint32_t* sprites;   // [n_sprites][32 * 32] RGBA: r | g << 8 | b << 16 | a << 24
    const uint32_t* statics;   // [4][32 * 32] RGB tiles: floor, wall, exit, void
    const uint8_t* pos;        // LLE_BUF_POS
    const uint32_t* gems;      // LLE_BUF_GEMS
    const uint32_t* beams;     // LLE_BUF_BEAMS
    const uint8_t* src_colour; // LLE_BUF_SRC_COLOUR
    const int64_t* env_ids;    // NULL: slot s renders env s
    void* out;
    int64_t pos_stride, pos_agent_stride, beam_stride, colour_stride;  // elements
    int64_t n_envs, envs_per_map;
    int64_t pitch;             // elements per frame
    int64_t frame_bytes;       // 3 (32H+1)(32W+1)
    int32_t H, W, A, env_sources;
    int32_t agent_base, n_agent_num, hlaser_base, vlaser_base, n_laser_num, source_base, n_source_num, gem_sprite;
};

__device__ __forceinline__ uint32_t blend(uint32_t bg, uint32_t fg, const float* alpha_of) {
    // add_transparent_image (renderer.rs:132-149): alpha = a / 255, ((1 - alpha) * bg + alpha * fg) as u8, every op rounded.  Plain
    // operators under the pragma above (and -ffp-contract=off): the __fmul_rn / __fadd_rn of the HIP headers are defined before any
    // pragma of this file and came out fused into an FMA, one unit off on some pixels.  alpha_of[a] = a / 255.0f, correctly rounded
    // (the kernel's LDS table: one division per lane and workgroup instead of one per blend).  a == 0 gives bg and a == 255 gives fg
    // exactly ((1 - 0) * bg + 0 * fg = bg; 255 / 255 = 1.0f: 0 * bg + 1 * fg = fg), so those pixels skip the arithmetic.
    const uint32_t a8 = fg >> 24;
    if (a8 == 0u) return bg;
    if (a8 == 255u) return fg & 0xFFFFFFu;
    const float a = alpha_of[a8];
    const float na = 1.0f - a;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float t0 = na * (float)((bg >> (8 * c)) & 255u);
        const float t1 = a * (float)((fg >> (8 * c)) & 255u);
        const float v = t0 + t1;
        out |= min(255u, (uint32_t)v) << (8 * c);  // `as u8`: truncation (saturating; never above 255 here)
    }
    return out;
}

template <typename T>
__device__ __forceinline__ void store_chunk(void* out, int64_t elem, const uint32_t (&w)[4]) {
    if constexpr (sizeof(T) == 1) {
        *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(out) + elem) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if constexpr (sizeof(T) == 4) {  // float32: 64 bytes
        float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + elem);
#pragma unroll
        for (int q = 0; q < 4; q++)
            dst[q] = make_float4((float)(w[q] & 255u), (float)((w[q] >> 8) & 255u), (float)((w[q] >> 16) & 255u), (float)(w[q] >> 24));
    } else {  // float16 / bfloat16: 32 bytes; 0..255 are exact in both
        uint32_t h[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t lo = (w[q >> 1] >> (16 * (q & 1))) & 255u, hi = (w[q >> 1] >> (16 * (q & 1) + 8)) & 255u;
            uint32_t blo, bhi;
            if constexpr (T::is_bf16) {  // bf16 = the upper half of the float32 (exact: 8 significant bits)
                blo = __float_as_uint((float)lo) >> 16;
                bhi = __float_as_uint((float)hi) >> 16;
            } else {
                blo = (uint32_t)__half_as_ushort(__float2half_rn((float)lo));
                bhi = (uint32_t)__half_as_ushort(__float2half_rn((float)hi));
            }
            h[q] = blo | bhi << 16;
        }
        uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(out) + elem);
        dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
        dst[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
}

struct F16Tag { static constexpr bool is_bf16 = false; uint16_t v; };
struct BF16Tag { static constexpr bool is_bf16 = true; uint16_t v; };

// One workgroup = one row of cells (32 pixel lines; the last row also the closing grid line) of one selected environment.
template <int DT>
__global__ __launch_bounds__(RENDER_THREADS) void render_kernel(RenderParams p) {
    extern __shared__ uint32_t lds_words[];
    __shared__ float alpha_of[256];
    static_assert(RENDER_THREADS == 256, "one alpha entry per lane");
    alpha_of[threadIdx.x] = (float)threadIdx.x / 255.0f;  // correctly rounded (HIP's default f32 division), like `as f32 / 255.0`
    const int W = p.W, H = p.H;
    uint16_t* draws = reinterpret_cast<uint16_t*>(lds_words);                    // [W][MAX_DRAWS]
    uint8_t* n_draws = reinterpret_cast<uint8_t*>(draws + (size_t)W * MAX_DRAWS);  // [W]
    uint8_t* tile_of = n_draws + W;                                               // [W]

    const int band = (int)(blockIdx.x % (uint32_t)H);
    const int64_t slot = (int64_t)(blockIdx.x / (uint32_t)H);
    int64_t env = p.env_ids ? p.env_ids[slot] : slot;
    const bool valid = env >= 0 && env < p.n_envs;
    if (!valid) env = 0;  // (reads stay in bounds; the frame is zeros)

    // ---- resolve the draw list of every cell of the row
    const uint32_t* tab = p.tables + p.map_off[env / p.envs_per_map];
    const uint32_t* ops = tab + (size_t)H * W;
    for (int j = threadIdx.x; j < W; j += RENDER_THREADS) {
        const uint32_t cw = tab[(size_t)band * W + j];
        uint16_t* d = draws + (size_t)j * MAX_DRAWS;
        int n = 0;
        const uint32_t n_ops = (cw >> 2) & 15u;
        for (uint32_t k = 0; k < n_ops; k++) {
            const uint32_t op = ops[(cw >> 6) + k];
            const uint32_t kind = op >> 30;
            if (kind == OP_LASER) {
                const uint32_t word = (op >> 8) & 31u, bit = (op >> 13) & 31u;
                if ((p.beams[env * p.beam_stride + word] >> bit) & 1u) {
                    const int colour = p.env_sources ? (int)p.src_colour[env * p.colour_stride + word] : (int)(op & 255u);
                    d[n++] = (uint16_t)(((op >> 18) & 1u ? p.vlaser_base : p.hlaser_base) + min(colour, p.n_laser_num));
                }
            } else if (kind == OP_GEM) {
                if (!((p.gems[env] >> (op & 31u)) & 1u)) d[n++] = (uint16_t)p.gem_sprite;
            } else {
                const int colour = p.env_sources ? (int)p.src_colour[env * p.colour_stride + ((op >> 8) & 31u)] : (int)(op & 255u);
                d[n++] = (uint16_t)(p.source_base + (int)((op >> 13) & 3u) * (p.n_source_num + 1) + min(colour, p.n_source_num));
            }
        }
        // agents after the cell's ops: a source's cell holds no agent, so the source stays last
        for (int a = 0; a < p.A && n < MAX_DRAWS; a++) {
            const uint8_t* q = p.pos + env * p.pos_stride + a * p.pos_agent_stride;
            if (q[0] == band && q[1] == j) d[n++] = (uint16_t)(p.agent_base + min(a, p.n_agent_num));
        }
        n_draws[j] = (uint8_t)n;
        tile_of[j] = (uint8_t)(cw & 3u);
    }
    __syncthreads();

    // ---- stream the band: 16 bytes of the HWC byte stream per lane and step
    const int64_t Wp = (int64_t)TILE * W + 1;
    const int64_t line = 3 * Wp;
    const int64_t lo = (int64_t)band * TILE * line;                 // a multiple of 96: chunks never straddle two bands
    const int64_t hi = band == H - 1 ? (p.frame_bytes + 15) & ~(int64_t)15 : lo + TILE * line;
    const int64_t n_px = p.frame_bytes / 3;
    void* out = p.out;
    const int64_t base = slot * p.pitch;
    for (int64_t b = lo + 16 * (int64_t)threadIdx.x; b < hi; b += 16 * RENDER_THREADS) {
        // 32-bit index arithmetic (a frame is < 2^32 bytes: 3 * 8161^2 at LLE_MAX_DIM): a 64-bit division is a long software sequence
        const uint32_t b32 = (uint32_t)b, px0 = b32 / 3u;
        const uint32_t r = b32 - 3u * px0;
        int y = (int)(px0 / (uint32_t)Wp), x = (int)(px0 - (uint32_t)y * (uint32_t)Wp);
        uint32_t rgb[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            uint32_t c = 0;
            if (valid && (int64_t)px0 + k < n_px) {
                if ((y & (TILE - 1)) == 0 || (x & (TILE - 1)) == 0) {
                    c = GRID_GREY;
                } else {
                    const int j = x >> 5, off = (y & (TILE - 1)) * TILE + (x & (TILE - 1));
                    c = p.statics[tile_of[j] * TILE_PX + off];
                    const uint16_t* d = draws + (size_t)j * MAX_DRAWS;
                    for (int q = 0, nq = n_draws[j]; q < nq; q++) c = blend(c, p.sprites[(size_t)d[q] * TILE_PX + off], alpha_of);
                }
            }
            rgb[k] = c;
            if (++x == Wp) { x = 0; y++; }
        }
        // 18 bytes of six pixels -> the 16 from byte r on
        uint32_t s[5];
        s[0] = (rgb[0] & 0xFFFFFFu) | rgb[1] << 24;
        s[1] = (rgb[1] >> 8 & 0xFFFFu) | (rgb[2] & 0xFFFFu) << 16;
        s[2] = (rgb[2] >> 16 & 0xFFu) | (rgb[3] & 0xFFFFFFu) << 8;
        s[3] = (rgb[4] & 0xFFFFFFu) | rgb[5] << 24;
        s[4] = rgb[5] >> 8 & 0xFFFFu;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = (uint32_t)((((uint64_t)s[q + 1] << 32) | s[q]) >> (8 * r));
        if constexpr (DT == LLE_RENDER_U8) store_chunk<uint8_t>(out, base + b, w);
        else if constexpr (DT == LLE_RENDER_F16) store_chunk<F16Tag>(out, base + b, w);
        else if constexpr (DT == LLE_RENDER_BF16) store_chunk<BF16Tag>(out, base + b, w);
        else store_chunk<float>(out, base + b, w);
    }
}

template __global__ void render_kernel<0>(RenderParams);
template __global__ void render_kernel<1>(RenderParams);
template __global__ void render_kernel<2>(RenderParams);
template __global__ void render_kernel<3>(RenderParams);

}  // namespace lle

// ================================================================================================ host side
using lle::RenderParams;
using namespace lle_abi_host;

namespace {

std::atomic<uint32_t> g_launched{0};
const char* const KERNEL_NAMES[4] = {"render_kernel<0>", "render_kernel<1>", "render_kernel<2>", "render_kernel<3>"};

struct MapStatics {
    int32_t H = 0, W = 0, A = 0, n_sources = 0;
    std::vector<uint32_t> words;  // [H*W] cell words, then the ops
};

uint32_t rgba_word(const uint8_t* px) { return px[0] | px[1] << 8 | px[2] << 16 | (uint32_t)px[3] << 24; }

// image::imageops::rotate90 (clockwise): dst[x][31 - y] = src[y][x]
void rotate90(const uint32_t* src, uint32_t* dst) {
    for (int y = 0; y < lle::TILE; y++)
        for (int x = 0; x < lle::TILE; x++) dst[x * lle::TILE + (lle::TILE - 1 - y)] = src[y * lle::TILE + x];
}

uint32_t host_blend(uint32_t bg, uint32_t fg) {  // renderer.rs:132-149 (contraction is off for this file)
    const float a = (float)(fg >> 24) / 255.0f;
    uint32_t out = 0;
    for (int c = 0; c < 3; c++) {
        const float b = (float)((bg >> (8 * c)) & 255u), f = (float)((fg >> (8 * c)) & 255u);
        const float na = 1.0f - a;
        const float t0 = na * b;
        const float t1 = a * f;
        const float v = t0 + t1;
        out |= std::min(255u, (uint32_t)v) << (8 * c);
    }
    return out;
}

// The draw ops of every cell of `map` (see the top of the file); `err` set on failure.
bool build_map(const lle_map* map, MapStatics& ms, std::string& err) {
    lle_map_info info{};
    if (lle_map_get_info(map, &info) != LLE_OK) { err = "lle_map_get_info failed"; return false; }
    ms.H = info.height; ms.W = info.width; ms.A = info.n_agents; ms.n_sources = info.n_sources;
    const int HW = ms.H * ms.W;
    auto positions = [&](int which) {
        std::vector<int32_t> ij((size_t)2 * std::max(0, lle_map_positions(map, which, nullptr, 0)));
        lle_map_positions(map, which, ij.data(), (int)ij.size() / 2);
        return ij;
    };
    std::vector<uint32_t> tile((size_t)HW, lle::TILE_FLOOR);
    std::vector<int> gem((size_t)HW, -1), source((size_t)HW, -1);
    // the static frame's order (renderer.rs:39-73): walls (sources included), exits, voids; a cell is one of them
    for (int w : {LLE_POS_WALL, LLE_POS_EXIT, LLE_POS_VOID}) {
        const auto ij = positions(w);
        const uint32_t t = w == LLE_POS_WALL ? lle::TILE_WALL : w == LLE_POS_EXIT ? lle::TILE_EXIT : lle::TILE_VOID;
        for (size_t k = 0; k + 1 < ij.size(); k += 2) tile[(size_t)ij[k] * ms.W + ij[k + 1]] = t;
    }
    const auto gij = positions(LLE_POS_GEM);
    for (size_t k = 0; k + 1 < gij.size(); k += 2) gem[(size_t)gij[k] * ms.W + gij[k + 1]] = (int)(k / 2);
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    std::vector<int> first_word(src.size());
    for (size_t s = 0, w = 0; s < src.size(); s++) {  // lle_map_info.n_beam_words: ceil(length / 32) words per source, at least one
        first_word[s] = (int)w;
        w += (size_t)std::max(1, (src[s].length + 31) / 32);
        source[(size_t)src[s].i * ms.W + src[s].j] = (int)s;
    }
    std::vector<lle_cell_layer> layers((size_t)std::max(0, lle_map_cell_layers(map, nullptr, 0)));
    lle_map_cell_layers(map, layers.data(), (int)layers.size());
    std::vector<std::vector<uint32_t>> stack((size_t)HW);  // laser ops of each cell, outermost first
    for (const auto& l : layers) {
        const lle_source_info& s = src[(size_t)l.laser_id];
        const uint32_t vertical = (l.direction == 0 || l.direction == 2) ? 1u : 0u;
        stack[(size_t)l.i * ms.W + l.j].push_back(lle::OP_LASER << 30 | vertical << 18 | (uint32_t)l.bit << 13 | (uint32_t)l.word << 8 |
                                                  ((uint32_t)s.agent_id & 255u));
    }
    ms.words.assign((size_t)HW, 0u);
    for (int c = 0; c < HW; c++) {
        std::vector<uint32_t> ops;
        const auto& st = stack[(size_t)c];
        const uint32_t gem_op = gem[(size_t)c] >= 0 ? lle::OP_GEM << 30 | (uint32_t)gem[(size_t)c] : 0u;
        // World::lasers() lists the outer layer and, when nested, the second one; draw_laser recurses from each to the bottom
        for (size_t e = 0; e < std::min<size_t>(st.size(), 2); e++) {
            for (size_t k = e; k < st.size(); k++) ops.push_back(st[k]);
            if (gem[(size_t)c] >= 0) ops.push_back(gem_op);  // draw_tile(Tile::Gem) under the stack
        }
        if (gem[(size_t)c] >= 0) ops.push_back(gem_op);  // the gem loop (renderer.rs:85-92)
        if (source[(size_t)c] >= 0) {
            const int s = source[(size_t)c];
            ops.push_back(lle::OP_SOURCE << 30 | (uint32_t)src[(size_t)s].direction << 13 | (uint32_t)first_word[(size_t)s] << 8 |
                          ((uint32_t)src[(size_t)s].agent_id & 255u));
        }
        if ((int)ops.size() > lle::MAX_CELL_OPS) { err = "a cell with more draw operations than the renderer holds"; return false; }
        const uint32_t first = (uint32_t)(ms.words.size() - (size_t)HW);
        ms.words[(size_t)c] = tile[(size_t)c] | (uint32_t)ops.size() << 2 | first << 6;
        ms.words.insert(ms.words.end(), ops.begin(), ops.end());
    }
    return true;
}

}  // namespace

struct lle_renderer {
    lle_batch* batch = nullptr;
    int device = 0;
    int n_maps = 0;
    int64_t n_envs = 0;
    std::vector<MapStatics> maps;
    std::vector<uint32_t> map_off;
    uint32_t* d_tables = nullptr;
    uint32_t* d_map_off = nullptr;
    uint32_t* d_sprites = nullptr;
    uint32_t* d_statics = nullptr;
    RenderParams p{};
};

namespace {

int upload_tables(lle_renderer* r, hipStream_t st) {
    std::vector<uint32_t> all;
    r->map_off.clear();
    for (const auto& m : r->maps) {
        r->map_off.push_back((uint32_t)all.size());
        all.insert(all.end(), m.words.begin(), m.words.end());
    }
    if (!r->d_tables) {
        if (hipMalloc(&r->d_tables, all.size() * 4) != hipSuccess || hipMalloc(&r->d_map_off, r->map_off.size() * 4) != hipSuccess)
            return fail(LLE_ERR_HIP, "hipMalloc of the render tables failed");
    }
    if (hipMemcpyAsync(r->d_tables, all.data(), all.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(r->d_map_off, r->map_off.data(), r->map_off.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(LLE_ERR_HIP, "uploading the render tables failed");
    return LLE_OK;
}

}  // namespace

extern "C" {

const char* lle_render_last_error(void) { return g_error.c_str(); }

void lle_render_free(lle_renderer* r) {
    if (!r) return;
    DeviceGuard g(r->device);
    (void)hipFree(r->d_tables);
    (void)hipFree(r->d_map_off);
    (void)hipFree(r->d_sprites);
    (void)hipFree(r->d_statics);
    delete r;
}

lle_renderer* lle_render_create(lle_batch* batch, const lle_map* const* maps, int n_maps, const lle_render_atlas* atlas, void* stream) {
    if (!batch || !maps || !atlas || !atlas->agents || !atlas->lasers || !atlas->sources || !atlas->gem || !atlas->void_) {
        fail(LLE_ERR_NULL, "NULL batch, maps or atlas");
        return nullptr;
    }
    if (n_maps != lle_batch_n_maps(batch) || atlas->n_agents < 0 || atlas->n_lasers < 0 || atlas->n_sources < 0) {
        fail(LLE_ERR_ARG, "n_maps must be lle_batch_n_maps(batch); sprite counts must not be negative");
        return nullptr;
    }
    lle_buffer_desc pos{}, gems{}, beams{}, colour{};
    if (lle_batch_get_buffer(batch, LLE_BUF_POS, &pos) || lle_batch_get_buffer(batch, LLE_BUF_GEMS, &gems) ||
        lle_batch_get_buffer(batch, LLE_BUF_BEAMS, &beams) || lle_batch_get_buffer(batch, LLE_BUF_SRC_COLOUR, &colour)) {
        fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
        return nullptr;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, pos.ptr) != hipSuccess) {
        fail(LLE_ERR_HIP, "the batch's buffers are not device memory");
        return nullptr;
    }
    auto* r = new lle_renderer();
    r->batch = batch;
    r->device = attr.device;
    r->n_maps = n_maps;
    r->n_envs = lle_batch_n_envs(batch);
    DeviceGuard g(r->device);
    std::string err;
    r->maps.resize((size_t)n_maps);
    for (int m = 0; m < n_maps; m++) {
        if (!maps[m] || !build_map(maps[m], r->maps[(size_t)m], err)) {
            fail(LLE_ERR_ARG, maps[m] ? err : "NULL map");
            delete r;
            return nullptr;
        }
        const MapStatics& a = r->maps[0], &b = r->maps[(size_t)m];
        if (a.H != b.H || a.W != b.W || a.A != b.A || a.n_sources != b.n_sources) {
            fail(LLE_ERR_ARG, "the maps of a batch share height, width, agents and sources");
            delete r;
            return nullptr;
        }
    }
    const MapStatics& m0 = r->maps[0];
    if (m0.W > 255 || m0.A > LLE_MAX_AGENTS) {
        fail(LLE_ERR_UNSUPPORTED, "map beyond the renderer's limits");
        delete r;
        return nullptr;
    }

    // ---- sprites: agents, horizontal lasers, vertical lasers, sources (N, E, S, W), gem
    const int na = atlas->n_agents, nl = atlas->n_lasers, ns = atlas->n_sources;
    const int n_sprites = (na + 1) + 2 * (nl + 1) + 4 * (ns + 1) + 1;
    if (n_sprites > 65535) {
        fail(LLE_ERR_ARG, "too many sprites");
        delete r;
        return nullptr;
    }
    std::vector<uint32_t> spr((size_t)n_sprites * lle::TILE_PX);
    auto load = [&](const uint8_t* src, uint32_t* dst) {
        for (int k = 0; k < lle::TILE_PX; k++) dst[k] = rgba_word(src + 4 * k);
    };
    RenderParams& p = r->p;
    int at = 0;
    p.agent_base = at;
    for (int k = 0; k <= na; k++, at++) load(atlas->agents + (size_t)k * lle::TILE_PX * 4, &spr[(size_t)at * lle::TILE_PX]);
    p.hlaser_base = at;
    for (int k = 0; k <= nl; k++, at++) load(atlas->lasers + (size_t)k * lle::TILE_PX * 4, &spr[(size_t)at * lle::TILE_PX]);
    p.vlaser_base = at;
    for (int k = 0; k <= nl; k++, at++) rotate90(&spr[(size_t)(p.hlaser_base + k) * lle::TILE_PX], &spr[(size_t)at * lle::TILE_PX]);
    p.source_base = at;
    // direction d (N=0 E=1 S=2 W=3) = the east-facing sprite turned (d + 3) % 4 times clockwise; RGB: alpha 255 (sprites.rs:70-88)
    std::vector<uint32_t> tmp(lle::TILE_PX), tmp2(lle::TILE_PX);
    for (int d = 0; d < 4; d++) {
        for (int k = 0; k <= ns; k++, at++) {
            load(atlas->sources + (size_t)k * lle::TILE_PX * 4, tmp.data());
            for (int t = 0; t < (d + 3) % 4; t++) {
                rotate90(tmp.data(), tmp2.data());
                tmp.swap(tmp2);
            }
            for (int q = 0; q < lle::TILE_PX; q++) spr[(size_t)at * lle::TILE_PX + q] = tmp[(size_t)q] | 0xFF000000u;
        }
    }
    p.gem_sprite = at;
    load(atlas->gem, &spr[(size_t)at * lle::TILE_PX]);
    p.n_agent_num = na;
    p.n_laser_num = nl;
    p.n_source_num = ns;

    // ---- static tiles (renderer.rs:39-73): floor, wall, exit (31 x 31 rectangle at (1, 1), thickness 2), void (blended)
    std::vector<uint32_t> stat((size_t)4 * lle::TILE_PX, lle::BACKGROUND_GREY);
    for (int k = 0; k < lle::TILE_PX; k++) {
        const int y = k / lle::TILE, x = k % lle::TILE;
        stat[(size_t)lle::TILE_WALL * lle::TILE_PX + k] = 0u;
        const bool rows = (y >= 1 && y <= 2) || (y >= 30 && y <= 31), cols = (x >= 1 && x <= 2) || (x >= 30 && x <= 31);
        if ((rows && x >= 1) || (cols && y >= 1)) stat[(size_t)lle::TILE_EXIT * lle::TILE_PX + k] = 0u;
        stat[(size_t)lle::TILE_VOID * lle::TILE_PX + k] = host_blend(lle::BACKGROUND_GREY, rgba_word(atlas->void_ + 4 * k));
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMalloc(&r->d_sprites, spr.size() * 4) != hipSuccess || hipMalloc(&r->d_statics, stat.size() * 4) != hipSuccess ||
        hipMemcpyAsync(r->d_sprites, spr.data(), spr.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(r->d_statics, stat.data(), stat.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
        fail(LLE_ERR_HIP, "uploading the sprites failed");
        lle_render_free(r);
        return nullptr;
    }
    if (upload_tables(r, st) != LLE_OK) {  // (synchronises: the host vectors above may go)
        lle_render_free(r);
        return nullptr;
    }
    p.tables = r->d_tables;
    p.map_off = r->d_map_off;
    p.sprites = r->d_sprites;
    p.statics = r->d_statics;
    p.pos = static_cast<const uint8_t*>(pos.ptr);
    p.pos_stride = pos.stride[0];
    p.pos_agent_stride = pos.ndim > 2 ? pos.stride[1] : 2;
    p.gems = static_cast<const uint32_t*>(gems.ptr);
    p.beams = static_cast<const uint32_t*>(beams.ptr);
    p.beam_stride = beams.ndim > 1 ? beams.stride[0] : 1;
    p.src_colour = static_cast<const uint8_t*>(colour.ptr);
    p.colour_stride = colour.ndim > 1 ? colour.stride[0] : 1;
    p.n_envs = r->n_envs;
    p.envs_per_map = r->n_envs / n_maps;
    p.H = m0.H;
    p.W = m0.W;
    p.A = m0.A;
    p.frame_bytes = 3 * (int64_t)(lle::TILE * m0.H + 1) * (lle::TILE * m0.W + 1);
    p.pitch = (p.frame_bytes + 127) & ~(int64_t)127;
    g_error.clear();
    return r;
}

int lle_render_update_map(lle_renderer* r, int map_index, const lle_map* map, void* stream) {
    if (!r || !map) return fail(LLE_ERR_NULL, "NULL renderer or map");
    if (map_index < 0 || map_index >= r->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    MapStatics ms;
    std::string err;
    if (!build_map(map, ms, err)) return fail(LLE_ERR_ARG, err);
    const MapStatics& old = r->maps[(size_t)map_index];
    if (ms.H != old.H || ms.W != old.W || ms.A != old.A || ms.n_sources != old.n_sources || ms.words.size() != old.words.size())
        return fail(LLE_ERR_ARG, "not a recompilation of the renderer's map");
    r->maps[(size_t)map_index] = std::move(ms);
    DeviceGuard g(r->device);
    return upload_tables(r, reinterpret_cast<hipStream_t>(stream));
}

int lle_render_desc_of(const lle_renderer* r, int64_t n_sel, int dtype, lle_render_desc* out) {
    if (!r || !out) return fail(LLE_ERR_NULL, "NULL renderer or descriptor");
    if (n_sel < 0 || dtype < LLE_RENDER_U8 || dtype > LLE_RENDER_F32) return fail(LLE_ERR_ARG, "bad n_sel or dtype");
    const int eb = dtype == LLE_RENDER_U8 ? 1 : dtype == LLE_RENDER_F32 ? 4 : 2;
    const int64_t Hp = lle::TILE * (int64_t)r->p.H + 1, Wp = lle::TILE * (int64_t)r->p.W + 1;
    *out = lle_render_desc{};
    out->elem_bytes = eb;
    out->ndim = 4;
    const int64_t shape[4] = {n_sel, Hp, Wp, 3}, stride[4] = {r->p.pitch, 3 * Wp, 3, 1};
    for (int k = 0; k < 4; k++) {
        out->shape[k] = shape[k];
        out->stride[k] = stride[k];
    }
    out->bytes = n_sel * r->p.pitch * eb;
    return LLE_OK;
}

int lle_render_frame(lle_renderer* r, const int64_t* env_ids_dev, int64_t n_sel, uint32_t flags, int dtype, void* out_dev,
                     int64_t out_bytes, void* stream) {
    if (!r || !out_dev) return fail(LLE_ERR_NULL, "NULL renderer or output");
    lle_render_desc d;
    const int rc = lle_render_desc_of(r, n_sel, dtype, &d);
    if (rc != LLE_OK) return rc;
    if (out_bytes < d.bytes) return fail(LLE_ERR_ARG, "output buffer smaller than lle_render_desc_of(...).bytes");
    if (reinterpret_cast<uintptr_t>(out_dev) % 16 != 0) return fail(LLE_ERR_ARG, "output buffer not 16-byte aligned");
    if ((flags & ~(uint32_t)LLE_RENDER_ENV_SOURCES) != 0) return fail(LLE_ERR_ARG, "unknown flags");
    if (n_sel == 0) return LLE_OK;
    if (!env_ids_dev && n_sel > r->n_envs) return fail(LLE_ERR_ARG, "n_sel > n_envs without env_ids");
    const int64_t blocks = n_sel * r->p.H;
    if (blocks > 0x7FFFFFFF) return fail(LLE_ERR_ARG, "too many frames for one launch");
    RenderParams p = r->p;
    p.env_ids = env_ids_dev;
    p.out = out_dev;
    p.env_sources = (flags & LLE_RENDER_ENV_SOURCES) ? 1 : 0;
    const size_t lds = (size_t)p.W * lle::MAX_DRAWS * 2 + 2 * (size_t)p.W;
    DeviceGuard g(r->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)blocks), block(lle::RENDER_THREADS);
    switch (dtype) {
        case LLE_RENDER_U8: hipLaunchKernelGGL(lle::render_kernel<0>, grid, block, lds, st, p); break;
        case LLE_RENDER_F16: hipLaunchKernelGGL(lle::render_kernel<1>, grid, block, lds, st, p); break;
        case LLE_RENDER_BF16: hipLaunchKernelGGL(lle::render_kernel<2>, grid, block, lds, st, p); break;
        default: hipLaunchKernelGGL(lle::render_kernel<3>, grid, block, lds, st, p); break;
    }
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "render launch failed");
    g_launched.fetch_or(1u << dtype);
    return LLE_OK;
}

size_t lle_render_debug_launched(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 4, g_launched.load(), buf, cap); }

}  // extern "C"
