// wino44_ups.hip -- nearest-x2 upsample + Conv2d(k3, s1, p1) (ldm Upsample, model.py:42-57) as a STRUCTURED Winograd F(4x4, 3x3) on
// fp32 MFMA, gfx950.
//
// For the layers AFTER the path's last integer decision only (dc_vic_amd.layers.allow_winograd(..., f44=True)): the three Upsample
// layers of the frozen VQGAN decoder.  A 4x4 output tile whose origin is a multiple of 4 reads the upsampled rows [a, b, b, c, c, d]
// (four low-resolution rows).  With the interpolation points 0, +-1, +-3/2, inf the B^T row of the point -1 is
// [0, 9/4, -9/4, -1, 1, 0]: zero on that pattern, so B^T P (P = the 6x4 row replication) keeps five rows,
//
//   S = [[9/4, -13/4, 1, 0], [0, -9/2, 2, 0], [0, -5/2, 5/2, 0], [0, 1/2, -1/2, 0], [0, 9/4, -13/4, 1]]   (points 0, 1, 3/2, -3/2, inf)
//
// and V = S d S^T of the 4x4 LOW-resolution patch d has 25 positions: 25 multiplies per 16 outputs and input channel (1.5625 per output;
// conv3x3_wino_ups_kernel, F(2x2): 2.25).  Every constant of S and of A^T is a dyadic rational (exact in fp32); G (fp64, at pack time)
// is the textbook Toom-Cook G of those points.
//
//   S x (4 -> 5):    t0 = 9/4 x0 - 13/4 x1 + x2    t1 = 2 x2 - 9/2 x1    t2 = 5/2 (x2 - x1)    t3 = -1/2 (x2 - x1)
//                    t4 = 9/4 x1 - 13/4 x2 + x3                                                                     (9 VALU)
//   A^T m (5 -> 4):  y0 = m0 + m1 + (m2 + m3)       y1 = m1 + 3/2 (m2 - m3)
//                    y2 = m1 + 9/4 (m2 + m3)        y3 = m1 + 27/8 (m2 - m3) + m4
//   G rows (the kept points 0, 1, 3/2, -3/2, inf): [4/9, 0, 0], [-2/5, -2/5, -2/5], [8/45, 4/15, 2/5], [8/45, -4/15, 2/5], [0, 0, 1]
//
// Engine of conv3x3_wino44_kernel (wino44.hip), with the changes the structure allows:
//   * one PERSISTENT workgroup per CU = 4 waves, one per SIMD; workgroup tile 64 output channels x 16 x 32 OUTPUT pixels = 32 tiles of
//     4x4, whose input is 8 + 2 low-resolution rows x 16 + 2 columns; a stage is 8 input channels = two k-steps = 100 MFMAs per wave.
//   * wave cg owns output channels 16 cg .. 16 cg + 15 of all 32 tiles and all 25 positions: 50 accumulators of 16x16 = 200 registers,
//     all in the accumulator file (two waves per SIMD would need <= 256 registers in all; the weights, operands and patch do not fit).
//   * pre-transformed weights straight from global memory into operand registers (six `global_load_dwordx4` + one `global_load_dword`
//     per k-step from the packed image [k-step 2][(group 6)[cg 4][k 4][m 16][4 positions] | [cg 4][k 4][m 16] (position 24)]).
//   * the raw low-resolution patch (8 ch x 10 rows x six 16-byte segments) by LDS-DMA, two pieces per wave and stage, two stages ahead.
//   * input transform: ONE 4x4 patch per thread and stage (12 LDS reads, column + row pass = 81 VALU, 7 stores into the V image
//     [k-step][(group 6)[block 2][k 4][n 16][4 positions] | [block 2][k 4][n 16] (position 24)]), three VALU behind every second MFMA.
//   * output transform A^T M A in registers; bias -> act -> (+ res) -> 16-byte stores; optional GroupNorm partials in the layout of
//     dcvic_conv3x3_wino44_stats_f32 (the 16 x 32-pixel tile grid of the output).
// LDS: 2 x 8 KiB raw patch + 2 x 25 KiB V + two bias rows = 66.5 KiB.
// Deterministic and batch-invariant: per position the reduction runs over the 4-channel k-steps ascending inside the MFMA's ordered fmaf
// chain; the tiling never depends on N.
#include "wino_stream.h"

#define U4_TH 16           // output tile rows / columns
#define U4_TW 32
#define U4_PW 24           // LDS row: low-resolution columns lx0 - 4 .. lx0 + 19 as six 16-byte segments; the patch's 18 columns at 3 .. 20
#define U4_PLANE 240       // 10 rows
#define U4_KC 8            // input channels per stage (two k-steps of four)
#define U4_SEGS 480        // float4 segments of a stage: 8 ch x 10 rows x 6
#define U4_XSLOTS 2
#define U4_XS 2048         // floats (512 lanes x 4: the last slot's idle lanes write zeros behind the patch)
#define U4_KUS 6400        // floats of one k-step's packed weights: 25 positions x 4 ch x 64 co
#define U4_US 12800
#define U4_KVS 3200        // floats of one k-step's V image: 25 positions x 4 ch x 32 tiles
#define U4_VS 6400
#define U4_CO 64
#define U4_THREADS 256
#define U4_OFF_V (2 * U4_XS)
#define U4_OFF_BIAS (U4_OFF_V + 2 * U4_VS)
#define U4_LDS_FLOATS (U4_OFF_BIAS + 2 * U4_CO)

// position p = 5 a + b holds row a, column b of S d S^T; groups 0..5 = positions 4g .. 4g + 3, position 24 on its own
__device__ __forceinline__ double u4_u(const float* g, int a, int b) {
    const double G[5][3] = {{4.0 / 9.0, 0.0, 0.0}, {-2.0 / 5.0, -2.0 / 5.0, -2.0 / 5.0}, {8.0 / 45.0, 4.0 / 15.0, 2.0 / 5.0},
                            {8.0 / 45.0, -4.0 / 15.0, 2.0 / 5.0}, {0.0, 0.0, 1.0}};
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) s += G[a][r] * (double)g[r * 3 + c] * G[b][c];
    return s;
}

// packed[cotile][chunk][k-step 2][ [group 6][cg 4][k 4][m 16][slot 4] | [cg 4][k 4][m 16] ]  <-  w[Cout][Cin][3][3]  (fp64, rounded once)
__global__ void wino44_ups_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int n_chunks, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int e = (int)(i % U4_KUS);
    long long r = i / U4_KUS;
    const int ks = (int)(r & 1); r >>= 1;
    const int chunk = (int)(r % n_chunks);
    const int cotile = (int)(r / n_chunks);
    int p, cg, k, m;
    if (e < 6144) {
        const int q = e & 1023;
        cg = q >> 8; k = (q >> 6) & 3; m = (q >> 2) & 15; p = (e >> 10) * 4 + (q & 3);
    } else {
        const int q = e - 6144;
        cg = q >> 6; k = (q >> 4) & 3; m = q & 15; p = 24;
    }
    const int co = cotile * U4_CO + cg * 16 + m, ci = chunk * U4_KC + 4 * ks + k;
    float v = 0.f;
    if (co < Cout && ci < Cin) v = (float)u4_u(w + ((long long)co * Cin + ci) * 9, p / 5, p % 5);
    wp[i] = v;
}

// one third (three VALU) of the 1-D input transform S x (4 -> 5) from X0..X3 into Y0..Y4; T[4] carries the intermediates
#define U4_S_THIRD(Q, X0, X1, X2, X3, Y0, Y1, Y2, Y3, Y4, T)                                      \
    do {                                                                                           \
        if constexpr ((Q) == 0) {                                                                  \
            T[0] = __builtin_fmaf(-3.25f, X1, X2);         /* x2 - 13/4 x1 */                      \
            T[1] = __builtin_fmaf(-3.25f, X2, X3);         /* x3 - 13/4 x2 */                      \
            T[2] = X2 - X1;                                                                        \
        } else if constexpr ((Q) == 1) {                                                           \
            Y0 = __builtin_fmaf(2.25f, X0, T[0]);                                                  \
            Y4 = __builtin_fmaf(2.25f, X1, T[1]);                                                  \
            T[3] = X2 + X2;                                                                        \
        } else {                                                                                   \
            Y1 = __builtin_fmaf(-4.5f, X1, T[3]);                                                  \
            Y2 = 2.5f * T[2];                                                                      \
            Y3 = -0.5f * T[2];                                                                     \
        }                                                                                          \
    } while (0)

// 1-D output transform A^T m (5 -> 4)
__device__ __forceinline__ void u4_at(float m0, float m1, float m2, float m3, float m4, float& y0, float& y1, float& y2, float& y3) {
    const float s = m2 + m3, d = m2 - m3;
    y0 = (m0 + m1) + s;
    y1 = __builtin_fmaf(1.5f, d, m1);
    y2 = __builtin_fmaf(2.25f, s, m1);
    y3 = __builtin_fmaf(3.375f, d, m1 + m4);
}

__global__ __launch_bounds__(U4_THREADS, 1) void conv3x3_wino44_ups_kernel(const ConvKArgs K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // 0..3

    const long long HW = (long long)K.H * K.W;                    // low-resolution input plane
    const long long HWo = (long long)K.Hfull * K.Wfull;           // output plane

    // ---- the workgroup's stage stream (wino_stream.h), tile index co-tile slowest (an XCD's L2 keeps its weight slab), tiles of the OUTPUT
    using Tiles = WinoTiles<false, U4_TH, U4_TW>;
    const Tiles T(K, tid);
    if (T.empty()) return;
    const int S = T.S, ntile = T.ntile(), total = T.total;
    // ---- raw-patch DMA: float4 segment e = tid + s*256 of [8 ch][10 low-resolution rows][6 segments]
    auto X = wino_x_stream<U4_XSLOTS, U4_THREADS, U4_KC>(T, HW, [&](int e, int oy0, int ox0) __attribute__((always_inline)) {
        int o = -1;
        if (e < U4_SEGS) {
            const int k = e / 60, r = e - k * 60;
            const int py = r / 6, seg = r - py * 6;
            const int iy = oy0 / 2 - 1 + py, ix = ox0 / 2 - 4 + 4 * seg;   // W % 4 == 0: a segment is entirely inside or outside the row
            if (iy >= 0 && iy < K.H && ix >= 0 && ix < K.W) o = (int)(k * HW) + iy * K.W + ix;
        }
        return o;
    });
    // ---- weights: this wave's slice of the packed image, straight into operand registers (U.p: slab of the NEXT stage)
    const int cg = wave;
    const unsigned u_voff = 16u * (unsigned)(cg * 64 + lane);     // groups 0..5: byte offset inside a 4 KiB (k-step, group) block
    const unsigned u_soff = 4u * (unsigned)(cg * 64 + lane);      // position 24
    WinoUStream<U4_US, Tiles> U(T);
    const float* wp_cur = U.p;
    U.advance();

    // ---- input transform: thread -> channel k = tid / 32 (k-step k / 4), tile t = tid % 32 (block t / 16, column n = t % 16 of the
    //      MFMA's B operand); tile (row ty = t / 8, column tx = t % 8) of the 4 x 8 tile grid = low-resolution rows 2 ty - 1 .. 2 ty + 2,
    //      columns 2 tx - 1 .. 2 tx + 2 of the workgroup's patch
    const int t_k = tid >> 5, t_t = tid & 31;
    const int t_blk = t_t >> 4, t_n = t_t & 15, t_ty = t_t >> 3, t_tx = t_t & 7;
    const unsigned t_src = 4u * (unsigned)(t_k * U4_PLANE + (2 * t_ty) * U4_PW + 2 * t_tx + 3);
    const unsigned t_dst = 4u * (unsigned)(U4_OFF_V + (t_k >> 2) * U4_KVS + (t_blk * 64 + (t_k & 3) * 16 + t_n) * 4);
    const unsigned t_dst1 = 4u * (unsigned)(U4_OFF_V + (t_k >> 2) * U4_KVS + 3072 + t_blk * 64 + (t_k & 3) * 16 + t_n);
    const unsigned op_v = 4u * (unsigned)(U4_OFF_V + lane * 4);
    const unsigned op_s = 4u * (unsigned)(U4_OFF_V + 3072 + lane);

    // 50 accumulators of 16x16 = 200 registers, all in the accumulator file; every MFMA is inline asm with "+a" operands and the
    // epilogue reads them with explicit v_accvgpr_read (as in wino44.hip: the builtin lets hipcc move them through VGPRs / scratch)
    f32x4 acc[25][2];                                             // [position][16-tile block]

    // the 4x4 patch of this thread: row r = (pl[r] | pm[r].x, pm[r].y | pr[r]); column pass -> cq[5][4], row pass -> vv[5][5]
    float pl[4], pr[4];
    f32x2 pm[4];
    float cq[5][4], vv[5][5];
    float tt[4];
    auto t_load = [&](auto r_, unsigned xaddr) {
        constexpr int r = decltype(r_)::value;
        float &l = pl[r], &rr = pr[r];
        f32x2& m = pm[r];
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(l) : "v"(xaddr), "n"(4 * (r * U4_PW)));
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(m) : "v"(xaddr), "n"(4 * (r * U4_PW + 1)));   // (8-byte aligned: column 4 + 2 tx)
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(rr) : "v"(xaddr), "n"(4 * (r * U4_PW + 3)));
    };
    auto t_col = [&](auto c_, auto q_) {                           // third q of the column pass of column c (over the four rows)
        constexpr int c = decltype(c_)::value, q = decltype(q_)::value;
        if constexpr (c == 0) U4_S_THIRD(q, pl[0], pl[1], pl[2], pl[3], cq[0][0], cq[1][0], cq[2][0], cq[3][0], cq[4][0], tt);
        else if constexpr (c == 1) U4_S_THIRD(q, pm[0].x, pm[1].x, pm[2].x, pm[3].x, cq[0][1], cq[1][1], cq[2][1], cq[3][1], cq[4][1], tt);
        else if constexpr (c == 2) U4_S_THIRD(q, pm[0].y, pm[1].y, pm[2].y, pm[3].y, cq[0][2], cq[1][2], cq[2][2], cq[3][2], cq[4][2], tt);
        else U4_S_THIRD(q, pr[0], pr[1], pr[2], pr[3], cq[0][3], cq[1][3], cq[2][3], cq[3][3], cq[4][3], tt);
    };
    auto t_row = [&](auto a_, auto q_) {                           // third q of the row pass of row a
        constexpr int a = decltype(a_)::value, q = decltype(q_)::value;
        U4_S_THIRD(q, cq[a][0], cq[a][1], cq[a][2], cq[a][3], vv[a][0], vv[a][1], vv[a][2], vv[a][3], vv[a][4], tt);
    };
    auto t_store = [&](auto i_, unsigned vaddr, unsigned vaddr1) { // i = 0..5: positions 4i .. 4i + 3; i = 6: position 24
        constexpr int i = decltype(i_)::value;
        if constexpr (i < 6) {
            const f32x4 v = f32x4{vv[(4 * i) / 5][(4 * i) % 5], vv[(4 * i + 1) / 5][(4 * i + 1) % 5], vv[(4 * i + 2) / 5][(4 * i + 2) % 5],
                                  vv[(4 * i + 3) / 5][(4 * i + 3) % 5]};
            asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(vaddr), "v"(v), "n"(i * 2048) : "memory");
        } else {
            const float v = vv[4][4];
            asm volatile("ds_write_b32 %0, %1" :: "v"(vaddr1), "v"(v) : "memory");
        }
    };
    f32x4 uA[2][6];                                               // [k-step][group]: four positions of this lane's (co, channel)
    float uS[2];                                                  // [k-step]: position 24
    f32x4 opB[3][2];                                              // [set][block]: four positions of this lane's (channel, tile)
    float opS[2][2];                                              // [k-step][block]: position 24
    auto u_load = [&](auto ks_, auto pg_, const float* slab) {     // U of (k-step, group) of the stage whose slab is given
        constexpr int ks = decltype(ks_)::value, pg = decltype(pg_)::value;
        if constexpr (pg < 6) {
            f32x4& dst = uA[ks][pg];
            const float* base = slab + ks * U4_KUS + pg * 1024;   // (uniform: scalar base + 32-bit lane offset, the saddr form)
            const unsigned vo = u_voff;
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(vo), "s"(base) : "memory");
        } else {
            float& dst = uS[ks];
            const float* base = slab + ks * U4_KUS + 6144;
            const unsigned vo = u_soff;
            asm volatile("global_load_dword %0, %1, %2" : "=v"(dst) : "v"(vo), "s"(base) : "memory");
        }
    };
    auto op_load = [&](auto G_, unsigned va, unsigned vs) {       // B operands of group G = 7 ks + pg of a stage
        constexpr int G = decltype(G_)::value, ks = G / 7, pg = G % 7;
        if constexpr (pg < 6) {
            constexpr int set = (6 * ks + pg) % 3;                // twelve vector groups per stage: three sets rotate across stages too
            f32x4 &b0 = opB[set][0], &b1 = opB[set][1];
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b0) : "v"(va), "n"(ks * 4 * U4_KVS + 1024 * (2 * pg)));
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b1) : "v"(va), "n"(ks * 4 * U4_KVS + 1024 * (2 * pg + 1)));
        } else {
            float &s0 = opS[ks][0], &s1 = opS[ks][1];
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(s0) : "v"(vs), "n"(ks * 4 * U4_KVS));
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(s1) : "v"(vs), "n"(ks * 4 * U4_KVS + 256));
        }
    };
    auto dma_x = [&](auto s_, int buf) {
        constexpr int sl = decltype(s_)::value;
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const float4*>(X.xp[sl]), (lds_ptr_t)(smem + buf * U4_XS + (wave * 64 + sl * U4_THREADS) * 4), 16, 0, 0);
    };

    // ---- epilogue of one tile, in registers: lane holds element (co = 16 cg + 4 (lane / 16) + r, tile = 16 blk + lane % 16) of all 25
    // positions.  A^T M A per (block, r): 5 column passes + 4 row passes, bias -> act -> (+ res) -> four 16-byte row stores.
    WinoTileCursor<U4_CO, Tiles> C(T, smem + U4_OFF_BIAS);        // compute stream: the tile, its bias row in [2][64] by tile parity
    const int e_n = lane & 15, lq = lane >> 4;
    const float neg_slope = K.act == DCVIC_ACT_RELU ? 0.f : K.act == DCVIC_ACT_LRELU02 ? 0.2f : 1.f;
    const bool has_res = K.res != nullptr;
    auto tile_epilogue = [&]() __attribute__((always_inline)) {
        const int cotile = C.cotile, n = C.n, oy0 = C.oy0, ox0 = C.ox0;
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");          // the inline-asm MFMAs' results are read below
        auto A = [&](auto idx_, auto blk_, int r) __attribute__((always_inline)) -> float {
            constexpr int idx = decltype(idx_)::value, blk = decltype(blk_)::value;
            float v;
            const float src = acc[idx][blk][r];
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(src));
            return v;
        };
        const int co0 = cotile * U4_CO + cg * 16 + 4 * lq;
        float bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = C.bias(cg * 16 + 4 * lq + r);
        float gs[4] = {0.f, 0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};   // GroupNorm partials of this lane's four channels
        dcvic_static_for<0, 2>([&](auto blk_) {
            const int t = decltype(blk_)::value * 16 + e_n;
            const int oy = oy0 + 4 * (t >> 3), ox = ox0 + 4 * (t & 7);
            const int rows = K.Hfull - oy;                        // output rows of this tile inside the image (2 or >= 4)
            const bool in_img = ox < K.Wfull && rows > 0;         // Wfull % 8 == 0: all four columns or none
            const long long pix = (long long)oy * K.Wfull + ox;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float tm[4][5];                                   // A^T M: [output row i][position column b]
                dcvic_static_for<0, 5>([&](auto b_) {
                    constexpr int b = decltype(b_)::value;
                    u4_at(A(std::integral_constant<int, b>{}, blk_, r), A(std::integral_constant<int, 5 + b>{}, blk_, r),
                          A(std::integral_constant<int, 10 + b>{}, blk_, r), A(std::integral_constant<int, 15 + b>{}, blk_, r),
                          A(std::integral_constant<int, 20 + b>{}, blk_, r), tm[0][b], tm[1][b], tm[2][b], tm[3][b]);
                });
                float y[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    u4_at(tm[i][0], tm[i][1], tm[i][2], tm[i][3], tm[i][4], y[i][0], y[i][1], y[i][2], y[i][3]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[i][j] += bv[r];
                }
                // activation: none / ReLU / LeakyReLU(0.2) only (host check) = one negative-side slope, branch-free
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[i][j] = y[i][j] > 0.f ? y[i][j] : neg_slope * y[i][j];
                if (in_img && co0 + r < K.Cout) {
                    float* const ob = K.out + (long long)n * K.out_bs + (long long)(co0 + r) * HWo + pix;
                    if (has_res) {
                        const float* const rb = K.res + (long long)n * K.res_bs + (long long)(co0 + r) * HWo + pix;
                        f32x4 rv[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) rv[i] = *reinterpret_cast<const f32x4*>(rb + (long long)min(i, rows - 1) * K.Wfull);   // (clamped row: in bounds)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) y[i][j] += rv[i][j];
                    }
                    if (K.gn_part != nullptr) {                   // statistics of exactly the values stored (fixed order: row, column)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < rows) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) { gs[r] += y[i][j]; gq[r] = __builtin_fmaf(y[i][j], y[i][j], gq[r]); }
                            }
                    }
                    if (rows >= 4) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ob + (long long)i * K.Wfull) = f32x4{y[i][0], y[i][1], y[i][2], y[i][3]};
                    } else {
#pragma unroll
                        for (int i = 0; i < 3; ++i)
                            if (i < rows) *reinterpret_cast<f32x4*>(ob + (long long)i * K.Wfull) = f32x4{y[i][0], y[i][1], y[i][2], y[i][3]};
                    }
                }
            }
        });
        if (K.gn_part) {
            // per (image, channel, 16 x 32 output tile) the sum and the sum of squares of the 512 stored values, in the layout and order of
            // conv3x3_wino44_kernel: 32 per lane, then the 16 lanes of a row (same four channels) by xor shuffles
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { gs[r] += __shfl_xor(gs[r], o, 64); gq[r] += __shfl_xor(gq[r], o, 64); }
            }
            if (e_n == 0) {
                const int pt = (oy0 / U4_TH) * K.tiles_x + ox0 / U4_TW;
                const int npt = K.tiles_x * K.tiles_y;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co0 + r < K.Cout)
                        *reinterpret_cast<f32x2*>(K.gn_part + (((long long)n * K.Cout + co0 + r) * npt + pt) * 2) = f32x2{gs[r], gq[r]};
            }
        }
    };

    // ---- pipeline
    // prologue: X(0) -> Xr[0], X(1) -> Xr[1], U(stage 0, k-step 0) -> uA[0] / uS[0]; every thread transforms its patch of stage 0 -> V[0]
    dcvic_static_for<0, U4_XSLOTS>([&](auto s_) { dma_x(s_, 0); });
    X.advance();
    if (total > 1) {
        dcvic_static_for<0, U4_XSLOTS>([&](auto s_) { dma_x(s_, 1); });
        X.advance();
    }
    dcvic_static_for<0, 7>([&](auto pg_) { u_load(std::integral_constant<int, 0>{}, pg_, wp_cur); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    WINO_FENCE();
    dcvic_static_for<0, 4>([&](auto r_) { t_load(r_, t_src); });
    WINO_WAIT_LDS();
    dcvic_static_for<0, 4>([&](auto c_) { dcvic_static_for<0, 3>([&](auto q_) { t_col(c_, q_); }); });
    dcvic_static_for<0, 5>([&](auto a_) { dcvic_static_for<0, 3>([&](auto q_) { t_row(a_, q_); }); });
    dcvic_static_for<0, 7>([&](auto i_) { t_store(i_, t_dst, t_dst1); });
    WINO_WAIT_LDS();
    __syncthreads();
    WINO_FENCE();
    op_load(std::integral_constant<int, 0>{}, op_v, op_s);

    // One stage = 14 operand groups G = 7 ks + pg (k-step, group): groups 0..5 of a k-step are 8 MFMAs (4 positions x 2 blocks), group 6
    // is 2 (position 24 x 2 blocks): 100 slots.  The body has NO run-time condition (past the end of the stream the loads re-fetch the
    // last slab / patch and the transform writes a V image nobody reads).
    //   in front of a group's MFMAs: wait for its B operands (lgkmcnt), request the next group's; group 7 (the second k-step) also waits
    //   for the weights loaded during the first (vmcnt);
    //   the stage BARRIER sits in front of the LAST group: every LDS read of this stage has returned, the transform's stores, this wave's
    //   DMA pieces and the next stage's first weights have landed; behind it the first B operands of stage s + 1 are requested.
    auto run_stage = [&](int s) __attribute__((always_inline)) {
        const int cur = s & 1, nxt = cur ^ 1;
        const unsigned va = op_v + (unsigned)(cur * U4_VS * 4), vs = op_s + (unsigned)(cur * U4_VS * 4);
        const unsigned xaddr = t_src + (unsigned)(nxt * U4_XS * 4);      // X(s + 1) lives in Xr[(s + 1) & 1]
        const unsigned vaddr = t_dst + (unsigned)(nxt * U4_VS * 4);      // V(s + 1)
        const unsigned vaddr1 = t_dst1 + (unsigned)(nxt * U4_VS * 4);
        dcvic_static_for<0, 14>([&](auto G_) {
            constexpr int G = decltype(G_)::value, ks = G / 7, pg = G % 7, set = (6 * ks + pg) % 3;
            if constexpr (G < 13) {
                if constexpr (G == 7) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                WINO_FENCE();
                op_load(std::integral_constant<int, G + 1>{}, va, vs);
            } else {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __syncthreads();
                WINO_FENCE();
                op_load(std::integral_constant<int, 0>{}, op_v + (unsigned)(nxt * U4_VS * 4), op_s + (unsigned)(nxt * U4_VS * 4));
            }
            WINO_FENCE();
            constexpr int NQ = pg < 6 ? 8 : 2;
            dcvic_static_for<0, NQ>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                if constexpr (pg < 6) {
                    constexpr int ps = q >> 1, blk = q & 1;
                    const float a_ = uA[ks][pg][ps], b_ = opB[set][blk][ps];
                    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc[pg * 4 + ps][blk]) : "v"(a_), "v"(b_));
                } else {
                    const float a_ = uS[ks], b_ = opS[ks][q];
                    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc[24][q]) : "v"(a_), "v"(b_));
                }
                WINO_FENCE();
                constexpr int h = (pg < 6 ? 8 * pg : 48) + q;     // slot inside the k-step, 0 .. 49
                constexpr int sl = 50 * ks + h;                   // 0 .. 99
                // memory: per k-step one DMA piece of X(s + 2) (slot 1), then the seven weight loads of the NEXT k-step (slots 5 .. 29):
                // during k-step 0 those of (s, k-step 1), during k-step 1 those of (s + 1, k-step 0)
                if constexpr (h == 1) dma_x(std::integral_constant<int, ks>{}, cur);
                if constexpr ((h & 3) == 1 && h >= 5 && h < 33) {
                    if constexpr (ks == 0) u_load(std::integral_constant<int, 1>{}, std::integral_constant<int, (h - 5) / 4>{}, wp_cur);
                    else u_load(std::integral_constant<int, 0>{}, std::integral_constant<int, (h - 5) / 4>{}, U.p);
                }
                // transform of X(s + 1): four row loads at slots 2, 3, 6, 7 (landed by the wait in front of group 1), 27 thirds of the column
                // (4) and row (5) passes at the even slots 10 .. 62, the seven stores at slots 64 .. 70
                if constexpr (sl < 8 && (sl & 3) >= 2) t_load(std::integral_constant<int, ((sl / 4) * 2 + (sl & 1))>{}, xaddr);
                if constexpr (sl >= 10 && sl < 64 && (sl & 1) == 0) {
                    constexpr int piece = (sl - 10) / 2, tr = piece / 3, third = piece % 3;
                    if constexpr (tr < 4) t_col(std::integral_constant<int, tr>{}, std::integral_constant<int, third>{});
                    else t_row(std::integral_constant<int, tr - 4>{}, std::integral_constant<int, third>{});
                }
                if constexpr (sl >= 64 && sl < 71) t_store(std::integral_constant<int, sl - 64>{}, vaddr, vaddr1);
                WINO_FENCE();
            });
        });
        WINO_FENCE();
    };
    {
        int s = 0;
        for (int t = 0; t < ntile; ++t) {
            // the accumulators are (re)defined HERE, outside the stage loop, and die in the epilogue (see wino44.hip)
#pragma unroll
            for (int i = 0; i < 25; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < S; ++c, ++s) {
                run_stage(s);
                if (s + 2 < total) X.advance();                   // the DMA of this stage fetched X(s + 2): on to X(s + 3)
                wp_cur = U.p;
                if (s + 2 < total) U.advance();                   // U.p: slab of stage s + 2
            }
            tile_epilogue();
            C.next_tile();
        }
    }
}

static const DcvicWinoPack U4_PACK = {U4_CO, U4_KC, U4_US};

extern "C" size_t dcvic_wino44_ups_packed_bytes(int Cin, int Cout) { return dcvic_wino_packed_bytes(U4_PACK, Cin, Cout); }

extern "C" int dcvic_wino44_ups_pack_f32(const float* w, float* packed, int Cin, int Cout, void* stream) {
    return dcvic_wino_pack("wino44_ups_pack", wino44_ups_pack_kernel, U4_PACK, w, packed, Cin, Cout, stream);
}

static int wino44_ups_launch(int Cin, int Cout, const float* packed, const dcvic_conv_io* io, float* gn_part, void* stream) {
    ConvKArgs K;
    if (const int rc = dcvic_wino_check("conv3x3_wino44_ups", DCVIC_OUT_X2, U4_PACK, Cin, Cout, packed, io, &K)) return rc;
    DCVIC_CHECK_ARG(io->act == DCVIC_ACT_NONE || io->act == DCVIC_ACT_RELU || io->act == DCVIC_ACT_LRELU02,
                    "conv3x3_wino44_ups: activation %d not supported (none / ReLU / LeakyReLU(0.2) only)", io->act);
    K.gn_part = gn_part;
    return dcvic_wino_run<conv3x3_wino44_ups_kernel>("conv3x3_wino44_ups", &K, U4_PACK, U4_TH, U4_TW, U4_THREADS, U4_LDS_FLOATS * sizeof(float), stream);
}

// Replaces dcvic_conv3x3_wino_ups_f32 (ldm Upsample, model.py:42-57) on the layers that allow F(4x4, 3x3)
extern "C" int dcvic_conv3x3_wino44_ups_f32(int Cin, int Cout, const float* packed, const dcvic_conv_io* io, void* stream) {
    return wino44_ups_launch(Cin, Cout, packed, io, nullptr, stream);
}

// The same, additionally writing the statistics of the GroupNorm that follows (ldm Normalize, model.py:38-39, the next ResnetBlock's
// norm1, model.py:117-133) in the layout of dcvic_conv3x3_wino44_stats_f32
extern "C" int dcvic_conv3x3_wino44_ups_stats_f32(int Cin, int Cout, const float* packed, const dcvic_conv_io* io, float* gn_part, void* stream) {
    DCVIC_CHECK_ARG(gn_part, "conv3x3_wino44_ups_stats: null statistics buffer");
    return wino44_ups_launch(Cin, Cout, packed, io, gn_part, stream);
}
