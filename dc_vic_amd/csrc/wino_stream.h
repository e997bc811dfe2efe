// wino_stream.h -- the persistent tile stream of the four Winograd kernels (wino.hip, wino44.hip, wino44_ups.hip).  Device code only.
//
// One PERSISTENT workgroup per CU walks its share of the launch's tiles; all stages (8-input-channel chunks) of all its tiles form ONE
// stream, so the loads of the next tile's first stages are in flight during the last stages and the (register-only) epilogue of the
// current tile and nothing drains at a tile boundary.  Three cursors run along that stream at different distances:
//   * the X stream (WinoXStream): the raw input patch by LDS-DMA, two stages ahead; per thread NS 16-byte segments, each a running
//     pointer into the current source (or the zero source for padding), advanced per stage, re-derived per source and per tile;
//   * the weight stream (WinoUStream): the stage's packed slab, one stage ahead;
//   * the compute stream (WinoTileCursor): the tile whose MFMAs run now, with its bias row staged in LDS by tile parity.
// A kernel owns what is specific to it: the patch geometry (one callable: segment number -> offset inside the stage's planes, or -1),
// the input / output transforms, the MFMA schedule and the epilogue arithmetic.
#pragma once
#include "conv_common.h"

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static __device__ float dcvic_wino_zero[16];   // zero-initialised: source of padded lanes

// All LDS traffic of the stage loops is inline asm with hand-placed `s_waitcnt lgkmcnt(0)`: hipcc guards every LDS access it can see with
// `s_waitcnt vmcnt(0)` while an LDS-DMA is in flight (it cannot prove the DMA's destination does not alias), which serialises a stage
// into "DMA latency + transform + MFMA" (measured on wino.hip: 52 % -> MFMA-busy).
#define WINO_FENCE() __builtin_amdgcn_sched_barrier(0)
#define WINO_WAIT_LDS() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); WINO_FENCE(); } while (0)

// The workgroup's share of the tile indices 0 .. K.nblocks - 1: XCD x = blockIdx.x % 8 owns the contiguous range [xs, xe), slot
// j = blockIdx.x / 8 of that XCD takes tiles first = xs + j, first + J, ...  A tile index is (cotile, image, tile row, tile column) with
// the co-tile FASTEST (F(2x2): the workgroups of one L2 share input patches and weight slabs) or SLOWEST (F(4x4): an XCD's range lies
// inside one or two co-tiles, whose weight slabs stay in its L2 for the whole launch); both orders were chosen by measurement.
template <bool CO_FASTEST, int TH, int TW>
struct WinoTiles {
    const ConvKArgs& K;
    const int tid, S, J;                                          // thread, stages per tile, stride of this workgroup's walk
    int first, xe, total, n_ptiles;                               // total: stages in the workgroup's stream
    __device__ __forceinline__ WinoTiles(const ConvKArgs& K_, int tid_) : K(K_), tid(tid_), S(K_.n_chunks), J((int)gridDim.x / NXCD) {
        const int nb = K.nblocks, q = nb / NXCD, r = nb % NXCD, x = (int)blockIdx.x % NXCD;
        const int xs = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
        xe = xs + (x < r ? q + 1 : q);
        first = xs + (int)blockIdx.x / NXCD;
        total = ntile() * S;
        n_ptiles = K.nblocks / K.n_cotiles;
    }
    __device__ __forceinline__ bool empty() const { return first >= xe; }   // (uniform: the whole workgroup leaves before any barrier)
    __device__ __forceinline__ int ntile() const { return (xe - first + J - 1) / J; }
    __device__ __forceinline__ int cotile_of(int b) const { return CO_FASTEST ? b % K.n_cotiles : b / n_ptiles; }
    __device__ __forceinline__ void decode(int b, int& cotile, int& n, int& oy0, int& ox0) const {   // (oy0, ox0): OUTPUT coordinates
        if constexpr (CO_FASTEST) { cotile = b % K.n_cotiles; b /= K.n_cotiles; }
        else { cotile = b / n_ptiles; b -= cotile * n_ptiles; }
        const int tile_x = b % K.tiles_x; b /= K.tiles_x;
        const int tile_y = b % K.tiles_y; b /= K.tiles_y;
        n = b; oy0 = tile_y * TH; ox0 = tile_x * TW;
    }
};

// Position of one cursor in the stream: tile index and stage inside the tile
struct WinoCounter {
    int b, next;
    template <class Tiles>
    __device__ __forceinline__ bool step(const Tiles& T) {        // on to the next stage; true: it is the first stage of a new tile
        if (++next != T.S) return false;
        next = 0; b += T.J;
        return true;
    }
};

// X stream.  NS segments per thread (segment e = tid + s * NT), KCH input channels per stage; seg(e, oy0, ox0) gives the offset of
// segment e inside the stage's KCH planes for the tile at output (oy0, ox0), or -1 for padding.  xp[s] is what the DMA of slot s reads.
template <int NS, int NT, int KCH, class Tiles, class Seg>
struct WinoXStream {
    const Tiles& T;
    const Seg seg;
    const long long HW, stride;                                   // input plane; floats between two stages of one source
    const float* xp[NS];
    int poff[NS];
    int left, n;                                                  // channels left in the current source, image
    WinoCounter c;
    __device__ __forceinline__ WinoXStream(const Tiles& T_, long long HW_, Seg seg_) : T(T_), seg(seg_), HW(HW_), stride((long long)KCH * HW_), left(0), n(0), c{T_.first, 0} { setup(); }
    __device__ __forceinline__ void rebase(int ch) {              // pointers for absolute input channel ch of image n: the three-source walk
        const ConvKArgs& K = T.K;
        int si = 0;
        if (ch >= K.srcC[0]) { ch -= K.srcC[0]; si = 1; if (ch >= K.srcC[1]) { ch -= K.srcC[1]; si = 2; } }
        const float* base = K.src[si] + (long long)n * K.src_bs[si] + (long long)ch * HW;
#pragma unroll
        for (int s = 0; s < NS; ++s) xp[s] = poff[s] >= 0 ? base + poff[s] : dcvic_wino_zero;
        left = K.srcC[si] - ch;
    }
    __device__ __forceinline__ void setup() {                     // first stage of tile c.b
        int cot, oy0, ox0;
        T.decode(c.b, cot, n, oy0, ox0);
#pragma unroll
        for (int s = 0; s < NS; ++s) poff[s] = seg(T.tid + s * NT, oy0, ox0);
        rebase(0);
    }
    __device__ __forceinline__ void advance() {                   // after the DMA of an X stage: on to the next stage of the stream
        if (c.step(T)) {
            if (c.b < T.xe) setup();
        } else {
            left -= KCH;
            if (left > 0) {
#pragma unroll
                for (int s = 0; s < NS; ++s) xp[s] += poff[s] >= 0 ? stride : 0ll;   // (padding lanes stay on the zero word)
            } else {
                rebase(c.next * KCH);
            }
        }
    }
};
template <int NS, int NT, int KCH, class Tiles, class Seg>
__device__ __forceinline__ WinoXStream<NS, NT, KCH, Tiles, Seg> wino_x_stream(const Tiles& T, long long HW, Seg seg) { return {T, HW, seg}; }

// Weight stream: p = the packed slab (US floats per stage, [cotile][chunk]) of the stream's current stage.  Uniform.
template <int US, class Tiles>
struct WinoUStream {
    const Tiles& T;
    const float* p;
    WinoCounter c;
    __device__ __forceinline__ explicit WinoUStream(const Tiles& T_) : T(T_), c{T_.first, 0} { setup(); }
    __device__ __forceinline__ void setup() { p = T.K.wp + (long long)T.cotile_of(c.b) * T.S * (long long)US; }
    __device__ __forceinline__ void advance() {
        if (c.step(T)) { if (c.b < T.xe) setup(); }
        else p += US;
    }
};

// Compute stream: the tile being accumulated, decoded, and its bias row in sbias[par][CO] (staged at the tile boundary, read at least
// one barrier later by the tile's epilogue)
template <int CO, class Tiles>
struct WinoTileCursor {
    const Tiles& T;
    float* const sbias;
    WinoCounter c;
    int par, cotile, n, oy0, ox0;
    __device__ __forceinline__ WinoTileCursor(const Tiles& T_, float* sbias_) : T(T_), sbias(sbias_), c{T_.first, 0}, par(0) { enter(); }
    __device__ __forceinline__ void enter() {
        T.decode(c.b, cotile, n, oy0, ox0);
        if (T.tid < CO) sbias[par * CO + T.tid] = T.K.bias != nullptr ? T.K.bias[min(T.cotile_of(c.b) * CO + T.tid, T.K.Cout - 1)] : 0.f;
    }
    __device__ __forceinline__ float bias(int co) const { return T.K.bias != nullptr ? sbias[par * CO + co] : 0.f; }   // co inside the co-tile
    __device__ __forceinline__ bool stage_done() { return ++c.next == T.S; }   // true: that was the tile's last stage
    __device__ __forceinline__ void next_tile() {                 // after the tile's epilogue
        c.next = 0; c.b += T.J; par ^= 1;
        if (c.b < T.xe) enter();
    }
};

// ---- F(2x2) helpers (both kernels of wino.hip)
// LDS-DMA of 16 bytes per lane in the saddr form, by hand (hipcc re-materialises 64-bit per-lane addresses inside the loop): uniform
// 64-bit base + 32-bit lane offset -> LDS byte address lds + 16 * lane -- 2.38 -> 2.32 ms on the 256 -> 256 @ 128^2 x 32 layer
__device__ __forceinline__ void wino_dma_saddr(const float* base, unsigned voff, unsigned lds) {
    const unsigned long long sb = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(reinterpret_cast<unsigned long long>(base) & 0xffffffffull)) & 0xffffffffull
                                | ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(reinterpret_cast<unsigned long long>(base) >> 32)) << 32);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sb), "s"(lds) : "memory", "m0");
}

// Output of one channel of a lane's 2x2 tile (y00 y01 / y10 y11, before the bias): bias -> act -> (+ res) -> ONE 16-byte store.
// Lanes tx and tx ^ 1 hold the 2x2 outputs of two horizontally adjacent tiles: they swap one row each (DPP quad_perm [1,0,3,2]) so that
// the even lane owns FOUR consecutive columns of the upper row and the odd lane of the lower row -- one 16-byte store (and residual
// load) per lane and channel instead of two 8-byte ones (VMEM instructions are the expensive part of these kernels' side work).
// dst / res: this lane's row segment; live: inside the image and the layer's channels.
__device__ __forceinline__ void wino22_store(float y00, float y01, float y10, float y11, float bias, int act, bool odd, f32x4 res, float* dst, bool live) {
    y00 = dcvic_act(y00 + bias, act); y01 = dcvic_act(y01 + bias, act);
    y10 = dcvic_act(y10 + bias, act); y11 = dcvic_act(y11 + bias, act);
    const float g0 = odd ? y00 : y10, g1 = odd ? y01 : y11;       // what the neighbour needs from this lane
    const float n0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, g0), 0xB1, 0xF, 0xF, true));
    const float n1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, g1), 0xB1, 0xF, 0xF, true));
    const f32x4 o = odd ? f32x4{n0, n1, y10, y11} : f32x4{y00, y01, n0, n1};
    if (live) *reinterpret_cast<f32x4*>(dst) = o + res;
}
