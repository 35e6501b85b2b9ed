// Backward of the sparse convolution (training path; the reference gets these
// from MinkowskiEngine's autograd functions behind every ME.Minkowski*Convolution*, train.py:194-206).
//
//   dX[i] = sum_k dY[j(i,k)] . W[k]^T   -> pcc_kernel_map_transpose + the forward kernel (pcc_conv_fwd) on
//                                          the transposed map with transposed weights: same MFMA loop.
//   dW[k] = sum_{(i,j) in map_k} X[i]^T dY[j]   -> conv_wgrad_kernel below (fp32 MFMA, rows are the GEMM's
//                                          K dimension), deterministic two-stage reduction.
//   db    = column sums of dY (caller).
//
// wgrad tiling: one workgroup owns kernel offset k, a 128 x 128 block of W[k] and every SPLIT-th group
// of 32 output rows (execution order of pcc_order_rows_by_mask; groups whose mask lacks k are
// skipped).  Per group the gathered X rows and the dY rows land in LDS as [chunk][row][32] images by
// buffer_load ... lds (absent neighbours: out-of-range offset -> zeros) and feed
// v_mfma_f32_32x32x2_f32 with A = X^T, B = dY: lane (r, h) reads X[row 2s+h][ch r] and dY[row 2s+h][co r] —
// two 128-B rows per ds_read_b32, all 64 banks once.  Single-buffered: 32 KB of LDS and 64
// accumulator registers per wave leave room for 4 workgroups per CU, which is what hides the
// index -> gather -> LDS round trips (no software pipeline).  Partials go to scratch
// [SPLIT][K][cin][cout]; a second kernel adds them in fixed order (bitwise reproducible).
// Roofline: MFMA fp32; algorithmic FLOPs = 2 * pairs * cin * cout, like the forward.
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace pcc {

constexpr int WG_SPLIT_MAX = 128;     // row-group splits per (offset, weight block): the grid must be many times the chip
                                      // (256 CUs x 5 workgroups) because offsets differ 3x in pair count (the centre has them all)
constexpr int WG_SPLIT_THIN = 256;     // the scalar kernel walks its rows serially: many short walks

__global__ __launch_bounds__(256) void map_transpose_kernel(const int32_t* __restrict__ nbr, int64_t n_out, int K,
                                                            int32_t* __restrict__ nbr_t, uint32_t* __restrict__ mask_t) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out * K) return;
    const int i = nbr[e];
    if (i < 0) return;
    const int k = (int)(e % K);
    nbr_t[(int64_t)i * K + k] = (int32_t)(e / K);
    atomicOr(&mask_t[i], 1u << k);
}

// Workgroups are dispatched in blockIdx order and an offset's pair count falls with its distance from the centre
// (the centre offset pairs every row, a corner offset a third of them): 3x3x3 kernels hand out the centre first,
// then faces, edges, corners, so that the launch ends on its cheapest workgroups.
__device__ __forceinline__ int wgrad_offset_of(int slot, int K) {
    constexpr unsigned char heavy_first[27] = {13, 4, 10, 12, 14, 16, 22, 1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25,
                                               0, 2, 6, 8, 18, 20, 24, 26};
    return K == 27 ? heavy_first[slot] : slot;
}

struct WgradArgs {
    const float* fin;
    const float* dy;
    const int32_t* nbr;      // [n_out, K] in execution order
    const int32_t* order;    // [n_out] execution position -> row of dy, or null
    const uint32_t* gmask;   // [ceil(n_out / 32)] or null
    float* partial;          // [splits, K, cin, cout]
    int64_t n_in, n_out;
    int cin, cout, K;
    int split;               // row-group splits (MFMA kernel)
};

// A wave's 32 x 32 accumulator tile (mfma32_row, common.h: row = input channel, col = output channel) -> rows ci0 .. ci0 + 31,
// column `co` (this lane's: tile column + r) of the partial image P [cin][cout]
__device__ __forceinline__ void store_partial_tile(const f32x16& acc, float* P, int cout, int ci0, int co, int h) {
    // one address per lane, the registers at wave-uniform distances from it: sixteen (row x cout) products, as 64-bit values in
    // vector registers across the stores, cost the slice kernels a wave per SIMD
    float* p = P + (int64_t)(ci0 + 4 * h) * cout + co;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) p[(int64_t)mfma32_row(reg) * cout] = acc[reg];
}

// ---- the pieces the four MFMA weight-gradient kernels share ----

// Roles of a thread in its 256-thread workgroup
struct WgradRoles {
    int lane, wave_u;     // lane of the wave; wave of the workgroup (wave-uniform)
    int r, h;             // MFMA role: lane (r, h) of the 32 x 32 tile (mfma32_row, common.h)
    int slot, rsub;       // DMA role: 8 lanes per row (16 bytes each), 8 rows per instruction
    int64_t ng;           // groups of 32 output rows
};
__device__ __forceinline__ WgradRoles wgrad_roles(int64_t n_out) {
    const int t = threadIdx.x, lane = t & 63;
    return {lane, __builtin_amdgcn_readfirstlane(t >> 6), lane & 31, lane >> 5, lane & 7, lane >> 3, (n_out + 31) >> 5};
}

// Buffer resource over a [rows][width] tensor: a voffset of BUF_OOB (any offset past the tensor) reads zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wgrad_rsrc(const float* p, int64_t rows, int width, int elem_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)(uint32_t)(rows * width * elem_bytes), BUF_FLAGS);
}
// Where this lane's 16 bytes of a row start (col_byte: the chunk's first column + the lane's slot, in bytes); zeros for an
// absent row or chunk
__device__ __forceinline__ uint32_t row_voffset(uint32_t row, bool present, uint32_t row_bytes, uint32_t col_byte) {
    return present ? row * row_bytes + col_byte : BUF_OOB;
}
// 16 bytes per lane into the LDS image at `lds_dst` (wave-uniform; lane l lands at byte 16 l): 8 rows of 128 B per instruction
__device__ __forceinline__ void stage16(__amdgpu_buffer_rsrc_t rsrc, const void* lds_dst, uint32_t voffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)lds_dst, 16, voffset, 0, 0, 0);
}

// The groups of a workgroup: s, s + SPLIT, ... in ascending order, of which only those whose mask holds one of the
// offsets in `want` are visited.  MASKS_PER_LOAD of their masks are inspected per load (one per lane) and balloted: a
// dependent scalar load per skipped group would cost ~1 us each.  A null gmask counts as all ones.
struct WgradWalk {
    static constexpr int MASKS_PER_LOAD = 64;
    const uint32_t* gmask;
    int64_t ng, gb;
    int split, lane;
    uint32_t want, gml;
    unsigned long long todo;
    __device__ __forceinline__ WgradWalk(const uint32_t* gmask_, int64_t ng_, int s, int split_, uint32_t offset_mask)
        : gmask(gmask_), ng(ng_), gb((int64_t)s - MASKS_PER_LOAD * (int64_t)split_), split(split_), lane(threadIdx.x & 63),
          want(offset_mask), gml(0u), todo(0ull) {}
    // once the loaded masks are used up (more() is false): the next MASKS_PER_LOAD masks, unless the groups are at_end()
    __device__ __forceinline__ void load() {
        gb += MASKS_PER_LOAD * (int64_t)split;
        if (at_end()) return;
        const int64_t gmine = gb + (int64_t)lane * split;
        gml = (gmine < ng) ? (gmask ? gmask[gmine] : 0xffffffffu) : 0u;
        todo = __ballot((gml & want) != 0u);
    }
    __device__ __forceinline__ bool at_end() const { return gb >= ng; }
    __device__ __forceinline__ bool more() const { return todo != 0ull; }
    // while more(): the next group and the offsets of `want` it holds (the same value in every lane)
    __device__ __forceinline__ void pop(int64_t& g, uint32_t& live) {
        const int bit = __ffsll(todo) - 1;
        todo &= todo - 1;
        g = gb + (int64_t)bit * split;
        live = (uint32_t)__shfl((int)gml, bit, 64) & want;
    }
    // All of it, for the kernels that fetch a group ahead; false, -1 and 0 when there is no further group.  The bf16 kernels
    // spell the two loops out, `for (load(); !at_end(); load()) while (more()) pop`: with the result of a call that changes the
    // walk as the condition of a loop around their MFMAs, hipcc keeps a second copy of every accumulator.
    __device__ __forceinline__ bool next(int64_t& g, uint32_t& live) {
        while (!more()) {
            load();
            if (at_end()) { g = -1; live = 0u; return false; }
        }
        pop(g, live);
        return true;
    }
};

__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                // [4 chunks][32 rows][32 ch]
    float* Bs = smem + 4 * 1024;     // [4 chunks][32 rows][32 co]
    const WgradRoles me = wgrad_roles(a.n_out);
    const int wave_u = me.wave_u;
    const int SPLIT = a.split;
    const int k = wgrad_offset_of(blockIdx.x / SPLIT, a.K), s = blockIdx.x % SPLIT;
    const int cin0 = blockIdx.y * 128, cout0 = blockIdx.z * 128;
    const int cbi = min(4, (a.cin - cin0) / 32), cbo = min(4, (a.cout - cout0) / 32);     // chunks present in this block
    // Blocks of at most 64 x 64 (64-channel layers) would leave three of the four waves without a tile and
    // half of the LDS images empty: there an iteration takes TWO row groups (waves 0-1 stage and consume the
    // first in image slots 0-1, waves 2-3 the second in slots 2-3), each wave multiplies 16 of its group's 32
    // rows into the whole 64 x 64 block, and every wave writes its own partial.
    const bool rowsplit = a.cin <= 64 && a.cout <= 64;       // a property of the layer, not of the block (host agrees)
    const int wm = rowsplit ? 0 : wave_u >> 1, wn = rowsplit ? 0 : wave_u & 1;           // 64 x 64 sub-block of the wave
    const int kp0 = rowsplit ? 8 * (wave_u & 1) : 0, kp1 = rowsplit ? kp0 + 8 : 16;
    const int cw = rowsplit ? (wave_u & 1) : wave_u;                                      // chunk this wave stages
    const int slotA = rowsplit ? 2 * (wave_u >> 1) : 2 * wm, slotB = rowsplit ? 2 * (wave_u >> 1) : 2 * wn;

    f32x16 acc[2][2] = {};

    const __amdgpu_buffer_rsrc_t rsrc_x = wgrad_rsrc(a.fin, a.n_in, a.cin, 4), rsrc_y = wgrad_rsrc(a.dy, a.n_out, a.cout, 4);
    const bool live_m[2] = {2 * wm < cbi, 2 * wm + 1 < cbi};
    const bool live_n[2] = {2 * wn < cbo, 2 * wn + 1 < cbo};

    WgradWalk walk(a.gmask, me.ng, s, SPLIT, 1u << k);
    auto take = [&](bool& any) -> int64_t {                // this wave's group of the next iteration
        int64_t g, g2 = -1;
        uint32_t one;                                      // 1u << k: nothing to choose from
        any = walk.next(g, one);
        if (rowsplit) {                                    // second group of the iteration (or none: zero images)
            if (any) walk.next(g2, one);
            if (wave_u >= 2) g = g2;
        }
        return g;
    };
    // The neighbour indices and dY rows of a group are fetched one iteration ahead, beside the previous group's
    // gathers: an iteration then waits for one memory round trip (the gathers), not for two in sequence.
    int idx[4];
    int64_t row[4];
    bool okr[4];
    auto load_rows = [&](int64_t g) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t pos = g * 32 + 8 * i + me.rsub;
            okr[i] = g >= 0 && pos < a.n_out;
            idx[i] = okr[i] ? a.nbr[pos * a.K + k] : -1;
            row[i] = okr[i] ? (a.order ? a.order[pos] : pos) : 0;
        }
    };
    bool any;
    int64_t g = take(any);
    load_rows(g);
    while (any) {
        // wave w stages one chunk of both operands: 4 instructions x 8 rows each
        uint32_t voa[4], vob[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            voa[i] = row_voffset(idx[i], idx[i] >= 0 && cw < cbi, a.cin * 4, (cin0 + cw * 32) * 4 + me.slot * 16);
            vob[i] = row_voffset(row[i], okr[i] && cw < cbo, a.cout * 4, (cout0 + cw * 32) * 4 + me.slot * 16);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            stage16(rsrc_x, As + wave_u * 1024 + i * 256, voa[i]);
            stage16(rsrc_y, Bs + wave_u * 1024 + i * 256, vob[i]);
        }
        g = take(any);
        load_rows(g);
        __syncthreads();
        const float* Ab = As + slotA * 1024 + me.h * 32 + me.r;
        const float* Bb = Bs + slotB * 1024 + me.h * 32 + me.r;
        for (int kp = kp0; kp < kp1; ++kp) {
            float av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = Ab[m * 1024 + kp * 64];
#pragma unroll
            for (int n = 0; n < 2; ++n) bv[n] = Bb[n * 1024 + kp * 64];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();
    }

    float* P = a.partial + ((int64_t)(rowsplit ? s * 4 + wave_u : s) * a.K + k) * a.cin * a.cout;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (!live_m[m]) continue;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (!live_n[n]) continue;
            store_partial_tile(acc[m][n], P, a.cout, cin0 + (2 * wm + m) * 32, cout0 + (2 * wn + n) * 32 + me.r, me.h);
        }
    }
#endif
}

// Slice kernel for the 64-channel class (the default for K = 27): what bounds these shapes is the byte rate of their
// gathers — every (X row, dY row) pair is 512 B for 8 k FLOP, twice the forward convolution's bytes per FLOP, and the
// measured rates (47-57 TFLOP/s) are the forward kernel's gather rate divided by two — so the tiling is chosen to move
// fewer bytes WITHOUT idling waves (round 2's four-offsets-per-workgroup kernel, one offset per wave, moved fewer bytes
// and idled the waves whose offset a group lacks: same time; removed in round 4):
//   * a workgroup owns the nine offsets of one dz plane and every SPLIT-th group of 32 output rows; the group's dY rows are
//     staged ONCE and reused by every offset of the plane that occurs in the group (about four of nine on a surface):
//     8 + 8 L KB per L offset-steps instead of 16 L;
//   * every wave works in every step: wave (m, n) owns the 32 x 32 tile (m, n) of the 64 x 64 block and keeps one
//     accumulator per offset of the plane (9 x 16 registers); a step = one (group, offset) = 16 MFMAs per wave;
//   * double-buffered images, the forward kernel's loop shape: the gathers of step s + 1 are issued before the MFMAs of
//     step s, the indices of step s + 2 are fetched beside them, one barrier per step.
// AHEAD = how many steps the gathers run in front of the MFMAs: 1 = two images per operand and __syncthreads() per step;
// 2 = three images, the step's wait is a counted s_waitcnt vmcnt(4) (everything but the newest four memory operations — the
// X gathers of the step after next and the index loads of the one after that, two each at least — has landed) + a bare
// s_barrier, so two steps' gathers are in flight per workgroup.
template <int O, int AHEAD>
__global__ __launch_bounds__(256) void conv_wgrad_slice_kernel(const WgradArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NB = AHEAD + 1;     // images per operand
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Xs = smem;                 // [NB][2 chunks][32 rows][32 ch]
    float* Ys = smem + NB * 2048;     // [NB][2 chunks][32 rows][32 co]
    const WgradRoles me = wgrad_roles(a.n_out);
    const int SPLIT = a.split;
    const int set = blockIdx.x / SPLIT, s = blockIdx.x % SPLIT;
    const int k0 = set * O;
    const uint32_t set_mask = (((1u << O) - 1u) << k0) & ((1u << a.K) - 1u);
    const int cbi = a.cin / 32, cbo = a.cout / 32;
    const int tm = me.wave_u >> 1, tn = me.wave_u & 1;            // my 32 x 32 tile of W[k]
    const bool tile_live = tm < cbi && tn < cbo;
    const int cw = me.wave_u & 1, rh = me.wave_u >> 1;            // my DMA role: chunk cw, rows 16 rh .. 16 rh + 15

    f32x16 acc[O] = {};

    const __amdgpu_buffer_rsrc_t rsrc_x = wgrad_rsrc(a.fin, a.n_in, a.cin, 4), rsrc_y = wgrad_rsrc(a.dy, a.n_out, a.cout, 4);

    // ---- step iterator: (group, offset) pairs of my groups, groups ascending, offsets ascending inside a group --------
    WgradWalk walk(a.gmask, me.ng, s, SPLIT, set_mask);
    int64_t it_g = -1;            // group of the pending offsets
    uint32_t it_rem = 0u;         // offsets of it_g not handed out yet
    int it_ysel = NB - 1;         // dY image of it_g (advances per group)
    struct Step { int64_t g; int o; int ysel; bool first; bool valid; };
    auto next_step = [&]() -> Step {
        Step st;
        st.first = false;
        if (it_rem == 0u) {
            if (!walk.next(it_g, it_rem)) { st.g = -1; st.o = k0; st.ysel = 0; st.valid = false; return st; }
            it_ysel = (it_ysel + 1 == NB) ? 0 : it_ysel + 1;
            st.first = true;
        }
        st.g = it_g;
        st.o = __builtin_ctz(it_rem);
        it_rem &= it_rem - 1u;
        st.ysel = it_ysel;
        st.valid = true;
        return st;
    };
    // indices of a step's rows (my two rows of the X image, and of the dY image when the step opens a group).  A valid
    // step always issues its two index loads (clamped addresses), whatever the lanes' rows: the counted wait relies on it.
    auto load_idx = [&](const Step& st, int (&idx)[2], int (&yrow)[2]) {
        if (!st.valid) {
            idx[0] = idx[1] = yrow[0] = yrow[1] = -1;
            return;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t pos = st.g * 32 + 16 * rh + 8 * i + me.rsub;
            const bool ok = pos < a.n_out;
            const int64_t pc = ok ? pos : a.n_out - 1;
            const int v = a.nbr[pc * a.K + st.o];
            idx[i] = ok ? v : -1;
            yrow[i] = -1;
            if (st.first) {
                const int yr = a.order ? a.order[pc] : (int)pc;
                yrow[i] = ok ? yr : -1;
            }
        }
    };
    auto issue = [&](const Step& st, int xbuf, const int (&idx)[2], const int (&yrow)[2]) {
        if (!st.valid) return;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            stage16(rsrc_x, Xs + xbuf * 2048 + cw * 1024 + (16 * rh + 8 * i) * 32,
                    row_voffset(idx[i], idx[i] >= 0 && cw < cbi, a.cin * 4, cw * 128 + me.slot * 16));
        if (st.first) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                stage16(rsrc_y, Ys + st.ysel * 2048 + cw * 1024 + (16 * rh + 8 * i) * 32,
                        row_voffset(yrow[i], yrow[i] >= 0 && cw < cbo, a.cout * 4, cw * 128 + me.slot * 16));
        }
    };
    auto compute = [&](const Step& st, int xbuf) {
        if (!tile_live) return;
        const float* Ab = Xs + xbuf * 2048 + tm * 1024 + me.h * 32 + me.r;
        const float* Bb = Ys + st.ysel * 2048 + tn * 1024 + me.h * 32 + me.r;
        const int oi = st.o - k0;
#define PCC_WG_CASE(I)                                                                                              \
    case I: {                                                                                                       \
        _Pragma("unroll") for (int kp = 0; kp < 16; ++kp)                                                           \
            acc[I < O ? I : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ab[kp * 64], Bb[kp * 64], acc[I < O ? I : 0], 0, 0, 0); \
    } break;
        switch (oi) {
            PCC_WG_CASE(0) PCC_WG_CASE(1) PCC_WG_CASE(2) PCC_WG_CASE(3) PCC_WG_CASE(4)
            PCC_WG_CASE(5) PCC_WG_CASE(6) PCC_WG_CASE(7) PCC_WG_CASE(8)
            default: break;
        }
#undef PCC_WG_CASE
    };

    int idxA[2], yrowA[2], idxB[2], yrowB[2];
    if constexpr (AHEAD == 1) {
        Step s0 = next_step();
        load_idx(s0, idxA, yrowA);
        issue(s0, 0, idxA, yrowA);                 // (waits for its own index loads)
        Step s1 = next_step();
        load_idx(s1, idxA, yrowA);
        __syncthreads();
        int xbuf = 0;
        while (s0.valid) {
            issue(s1, xbuf ^ 1, idxA, yrowA);
            Step s2 = next_step();
            load_idx(s2, idxB, yrowB);
            compute(s0, xbuf);
            __syncthreads();                       // vmcnt(0): step s1's images and step s2's indices have landed; s0's images are free
            s0 = s1;
            s1 = s2;
#pragma unroll
            for (int i = 0; i < 2; ++i) { idxA[i] = idxB[i]; yrowA[i] = yrowB[i]; }
            xbuf ^= 1;
        }
    } else {
        Step s0 = next_step();
        load_idx(s0, idxA, yrowA);
        issue(s0, 0, idxA, yrowA);
        Step s1 = next_step();
        load_idx(s1, idxA, yrowA);
        issue(s1, 1, idxA, yrowA);
        Step s2 = next_step();
        load_idx(s2, idxA, yrowA);                 // stays in registers until its gathers are issued in the loop
        int xb0 = 0;                               // image of s0; s1 = xb0 + 1, s2 = xb0 + 2 (mod 3)
        while (s0.valid) {
            Step s3 = next_step();
            load_idx(s3, idxB, yrowB);
            // all but the newest four memory operations have landed: newer than s0's gathers are s2's index loads (older
            // than the four), s1's gathers (>= 2) and s3's index loads (2)
            if (s1.valid && s3.valid) __builtin_amdgcn_s_waitcnt(0x0074);
            else __builtin_amdgcn_s_waitcnt(0x0070);
            __builtin_amdgcn_s_barrier();
            issue(s2, xb0 == 0 ? 2 : xb0 - 1, idxA, yrowA);
            compute(s0, xb0);
            s0 = s1;
            s1 = s2;
            s2 = s3;
#pragma unroll
            for (int i = 0; i < 2; ++i) { idxA[i] = idxB[i]; yrowA[i] = yrowB[i]; }
            xb0 = (xb0 == 2) ? 0 : xb0 + 1;
        }
    }

    if (!tile_live) return;
#pragma unroll
    for (int o = 0; o < O; ++o) {
        if (k0 + o >= a.K) break;
        store_partial_tile(acc[o], a.partial + ((int64_t)s * a.K + (k0 + o)) * a.cin * a.cout, a.cout, tm * 32, tn * 32 + me.r, me.h);
    }
#endif
}

// bf16 operands (pcc_conv_wgrad_bf16; cin, cout multiples of 64): X and dY are bf16, products accumulate in fp32 on
// v_mfma_f32_32x32x16_bf16.  The GEMM's K dimension is the ROWS, but the LDS images are [row][64 channels]
// (128-B rows, what the 16-B-per-lane LDS-DMA produces), so a lane's 8 consecutive k-values of one channel sit
// 128 B apart.  gfx950's transposing LDS read does the operand transpose: ds_read_b64_tr_b16 takes, per 16-lane
// group, a block of 4 rows x 16 columns (lane 4q+p addresses row q, columns 4p..4p+3) and hands lane i the 4 rows
// of column i — two of them make one MFMA operand (8 two-byte reads plus packing without it: 2.2x slower).
// Rows 128 B apart put rows q and q+2 on the same banks: the reads are 2-way conflicted, which hides under the
// gathers the kernel is bound by.
// A workgroup owns offset k, a block of up to 128 x 128 of W[k] = TM x TN tiles of 32 x 32 dealt round-robin to the
// four waves (128 x 128: a wave holds one column of 4 tiles and reads its dY operand once), and every SPLIT-th
// group of 32 rows (two MFMA k-steps).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// One MFMA operand (8 k-values = image rows of my column) from two transposing reads, 4 rows each: `p` = my address inside the
// first 4-row block (tr_off below), the second block four 128-B rows on
__device__ __forceinline__ bf16x8 tr_operand(const unsigned short* p) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p + 4 * 64));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
// transposing read: my address inside a 4-row x 16-column block, and the block's first column within the tile
__device__ __forceinline__ int tr_lane_offset(int lane) { return (((lane & 15) >> 2) * 64) + 16 * ((lane >> 4) & 1) + 4 * (lane & 3); }

__global__ __launch_bounds__(256) void conv_wgrad_bf16_kernel(const WgradArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* As = reinterpret_cast<unsigned short*>(smem);             // [2 chunks][32 rows][64 ch]
    unsigned short* Bs = As + 2 * 2048;                                       // [2 chunks][32 rows][64 co]
    const WgradRoles me = wgrad_roles(a.n_out);
    const int wave_u = me.wave_u;
    const int SPLIT = a.split;
    const int k = wgrad_offset_of(blockIdx.x / SPLIT, a.K), s = blockIdx.x % SPLIT;
    const int cin0 = blockIdx.y * 128, cout0 = blockIdx.z * 128;
    const int cbi = min(2, (a.cin - cin0) / 64), cbo = min(2, (a.cout - cout0) / 64);     // 64-channel chunks present
    const int TM = 2 * cbi, TN = 2 * cbo, NTILES = TM * TN;
    // 64 x 64 blocks fill one image slot per operand: the other slot takes a SECOND row group per iteration (waves
    // 0 / 2 stage the first group's X / dY, waves 1 / 3 the second's), doubling the MFMA work per barrier pair
    const bool two_groups = cbi == 1 && cbo == 1;

    f32x16 acc[4] = {};

    const __amdgpu_buffer_rsrc_t rsrc_x = wgrad_rsrc(a.fin, a.n_in, a.cin, 2), rsrc_y = wgrad_rsrc(a.dy, a.n_out, a.cout, 2);
    // staging roles: waves 0-1 the X chunks 0-1, waves 2-3 the dY chunks 0-1
    const bool stage_x = wave_u < 2;
    const int cw = wave_u & 1;
    // my tiles: t = wave, wave + 4, ...; tile t -> (m = t / TN, n = t % TN)
    int tm[4], tn[4];
    bool live[4];
    const int tr_off = tr_lane_offset(me.lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tt = wave_u + 4 * i;
        live[i] = tt < NTILES;
        tm[i] = live[i] ? tt / TN : 0;
        tn[i] = live[i] ? tt % TN : 0;
    }

    WgradWalk walk(a.gmask, me.ng, s, SPLIT, 1u << k);
    int64_t g;
    uint32_t one;                                              // 1u << k: nothing to choose from
    for (walk.load(); !walk.at_end(); walk.load()) while (walk.more()) {
        walk.pop(g, one);
        bool second = false;
        if (two_groups) {
            int64_t g2 = -1;
            second = walk.more();
            if (second) walk.pop(g2, one);
            if (cw == 1) g = g2;                           // waves 1 and 3 stage the second group (chunk 0 of it), or zeros
        }
        const int chunk = two_groups ? 0 : cw;
        uint32_t vo[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t pos = g * 32 + 8 * i + me.rsub;
            const bool ok = g >= 0 && pos < a.n_out;
            if (stage_x) {
                const int idx = ok ? a.nbr[pos * a.K + k] : -1;
                vo[i] = row_voffset(idx, idx >= 0 && chunk < cbi, a.cin * 2, (cin0 + chunk * 64) * 2 + me.slot * 16);
            } else {
                const int64_t row = ok ? (a.order ? a.order[pos] : pos) : 0;
                vo[i] = row_voffset(row, ok && chunk < cbo, a.cout * 2, (cout0 + chunk * 64) * 2 + me.slot * 16);
            }
        }
        unsigned short* dst = (stage_x ? As : Bs) + cw * 2048;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (stage_x) stage16(rsrc_x, dst + i * 512, vo[i]);
            else stage16(rsrc_y, dst + i * 512, vo[i]);
        }
        __syncthreads();
        const int nks = (two_groups && second) ? 4 : 2;
        for (int ks4 = 0; ks4 < nks; ++ks4) {                  // rows 16 ks + 8 h + j of group slot gs
            const int ks = ks4 & 1, gs = ks4 >> 1;
            const int row0 = 16 * ks + 8 * me.h;                // first of my 8 rows (k-values) in this MFMA step
            bf16x8 bop;
            int bn_loaded = -1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!live[i]) continue;                         // wave-uniform: EXEC stays all ones for the transposing reads
                const bf16x8 aop = tr_operand(As + ((tm[i] >> 1) + gs) * 2048 + row0 * 64 + (tm[i] & 1) * 32 + tr_off);
                if (tn[i] != bn_loaded) {                      // 128 x 128: all of the wave's tiles share n
                    bop = tr_operand(Bs + ((tn[i] >> 1) + gs) * 2048 + row0 * 64 + (tn[i] & 1) * 32 + tr_off);
                    bn_loaded = tn[i];
                }
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aop, bop, acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    float* P = a.partial + ((int64_t)s * a.K + k) * a.cin * a.cout;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!live[i]) continue;
        store_partial_tile(acc[i], P, a.cout, cin0 + tm[i] * 32, cout0 + tn[i] * 32 + me.r, me.h);
    }
#endif
}

// A pipelined form of this kernel (two or three image sets, the gathers of the next one / two row groups issued before the
// MFMAs of the current one, one barrier per group — the slice kernel's loop shape) was built and measured in round 2: SLOWER,
// 850 k-row shell 128 x 128: 264 TFLOP/s single-buffered, 240 with two image sets, 191 with three (64 x 64: 126 / 116 / 91).
// At 4.1 TB/s of 256-byte gathers the kernel sits at the gather rate of the memory system; what keeps that rate up is the
// number of workgroups per CU (16 KB of LDS each), which every extra image set cuts.
// 64 -> 64 with bf16 operands and 27 offsets: a row pair is 2 x 128 B for 8 k FLOP and the kernel above runs at the gather rate
// of the memory system (~4 TB/s of rows), so the only lever is bytes: a workgroup owns O consecutive offsets and a group's
// 32 dY rows are staged ONCE for all of the O that occur in the group (4 + 4 L KB per L live offsets instead of 8 L), each
// offset's X rows in its own image.  Single-buffered like the kernel above (occupancy carries the latency): one staging
// instruction per thread and image — wave w stages rows 8 w .. 8 w + 7 of every image — then wave (tm, tn) runs its 32 x 32
// tile of every live offset against the shared dY operand: per MFMA k-step one dY fragment, L X fragments, L MFMAs.
template <int O>
__global__ __launch_bounds__(256) void conv_wgrad_bf16_slice_kernel(const WgradArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* Xs = reinterpret_cast<unsigned short*>(smem);             // [O][32 rows][64 ch]
    unsigned short* Ys = Xs + O * 2048;                                       // [32 rows][64 co]
    const WgradRoles me = wgrad_roles(a.n_out);
    const int wave_u = me.wave_u;
    const int SPLIT = a.split;
    const int set = blockIdx.x / SPLIT, s = blockIdx.x % SPLIT;
    const int k0 = set * O;
    const uint32_t set_mask = (((1u << O) - 1u) << k0) & ((1u << a.K) - 1u);
    const int tm = wave_u >> 1, tn = wave_u & 1;

    f32x16 acc[O] = {};

    const __amdgpu_buffer_rsrc_t rsrc_x = wgrad_rsrc(a.fin, a.n_in, a.cin, 2), rsrc_y = wgrad_rsrc(a.dy, a.n_out, a.cout, 2);
    const int tr_off = tr_lane_offset(me.lane);

    WgradWalk walk(a.gmask, me.ng, s, SPLIT, set_mask);
    int64_t g;
    uint32_t live;
    for (walk.load(); !walk.at_end(); walk.load()) while (walk.more()) {
        walk.pop(g, live);
        const uint32_t rem = (uint32_t)__builtin_amdgcn_readfirstlane((int)(live >> k0));
        const int64_t pos = g * 32 + 8 * wave_u + me.rsub;
        const bool ok = pos < a.n_out;
        const int yrow = ok ? (a.order ? a.order[pos] : (int)pos) : -1;
        stage16(rsrc_y, Ys + wave_u * 512, row_voffset(yrow, yrow >= 0, a.cout * 2, me.slot * 16));
#pragma unroll
        for (int o = 0; o < O; ++o) {
            if (!((rem >> o) & 1u)) continue;
            const int idx = ok ? a.nbr[pos * a.K + k0 + o] : -1;
            stage16(rsrc_x, Xs + o * 2048 + wave_u * 512, row_voffset(idx, idx >= 0, a.cin * 2, me.slot * 16));
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int row0 = 16 * ks + 8 * me.h;
            const bf16x8 bop = tr_operand(Ys + row0 * 64 + tn * 32 + tr_off);
#pragma unroll
            for (int o = 0; o < O; ++o) {
                if (!((rem >> o) & 1u)) continue;                       // wave-uniform: EXEC stays all ones
                acc[o] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_operand(Xs + o * 2048 + row0 * 64 + tm * 32 + tr_off), bop, acc[o], 0, 0, 0);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int o = 0; o < O; ++o) {
        if (k0 + o >= a.K) break;
        store_partial_tile(acc[o], a.partial + ((int64_t)s * a.K + (k0 + o)) * a.cin * a.cout, a.cout, tm * 32, tn * 32 + me.r, me.h);
    }
#endif
}

// thin shapes (cin or cout not a multiple of 32: q-map branches, input layer, narrow heads): cin * cout <= 4096.
// One workgroup per (offset, split).  With >= 256 (ci, co) pairs a thread owns up to 16 pairs and walks the
// split's rows; with fewer pairs (64 -> 1: the occupancy head on 5 M candidates) the spare threads take
// every RL-th row instead and the row lanes are summed through LDS at the end.
__global__ __launch_bounds__(256) void conv_wgrad_thin_kernel(const WgradArgs a) {
    __shared__ float red[256];
    const int k = blockIdx.x / WG_SPLIT_THIN, s = blockIdx.x % WG_SPLIT_THIN;
    const int pairs = a.cin * a.cout;
    int pp = 1;
    while (pp < pairs && pp < 256) pp <<= 1;              // pairs rounded up to a power of two, at most 256
    const int RL = 256 / pp;                                // row lanes (1 when pairs >= 256)
    const int pid = threadIdx.x % pp, rl = threadIdx.x / pp;
    float acc[16];
    int ci[16], co[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        acc[q] = 0.0f;
        const int e = min(pid + 256 * q, pairs - 1);
        ci[q] = e / a.cout;
        co[q] = e - ci[q] * a.cout;
    }
    const int64_t per = (a.n_out + WG_SPLIT_THIN - 1) / WG_SPLIT_THIN;
    const int64_t lo = s * per, hi = min(a.n_out, lo + per);
    for (int64_t pos = lo + rl; pos < hi; pos += RL) {
        const int idx = a.nbr[pos * a.K + k];
        if (idx < 0) continue;
        const int64_t row = a.order ? a.order[pos] : pos;
        const float* x = a.fin + (int64_t)idx * a.cin;
        const float* y = a.dy + row * a.cout;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (256 * q < pairs) acc[q] = fmaf(x[ci[q]], y[co[q]], acc[q]);
        }
    }
    float* P = a.partial + ((int64_t)s * a.K + k) * pairs;
    if (RL > 1) {                                           // pairs < 256: only acc[0] is in use
        red[threadIdx.x] = acc[0];
        __syncthreads();
        if (rl == 0 && pid < pairs) {
            float sum = 0.0f;
            for (int l = 0; l < RL; ++l) sum += red[l * pp + pid];        // fixed order
            P[pid] = sum;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = threadIdx.x + 256 * q;
        if (e < pairs) P[e] = acc[q];
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int64_t elems, int nsplit,
                                                           float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    float sum = 0.0f;
    for (int s = 0; s < nsplit; ++s) sum += partial[(int64_t)s * elems + e];        // fixed order
    dw[e] = sum;
}

// the same sums, four elements per thread with 16-byte loads (elems % 4 == 0, 16-byte aligned partials: the MFMA shapes)
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(const float4* __restrict__ partial, int64_t elems4, int nsplit,
                                                            float4* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems4) return;
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int s = 0; s < nsplit; ++s) {                                              // fixed order
        const float4 v = partial[(int64_t)s * elems4 + e];
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
    }
    dw[e] = sum;
}

// The legal values of an A/B switch, the default first.  pick() reads the switch; dispatch() hands the matching value to `f` as
// a compile-time constant (std::integral_constant): template instances come from the same list as the switch's legal values.
template <int... V>
struct Choices {
    static int pick(const char* env_name) {
        const char* e = getenv(env_name);
        const int v = e ? atoi(e) : -1, all[] = {V...};
        return ((v == V) || ...) ? v : all[0];
    }
    template <class F>
    static void dispatch(int v, F&& f) { ((v == V ? f(std::integral_constant<int, V>{}) : void()), ...); }
};

}  // namespace pcc

using namespace pcc;

extern "C" {

int pcc_kernel_map_transpose(const int32_t* nbr, int64_t n_out, int32_t K, int64_t n_in, int32_t* nbr_t, uint32_t* row_mask_t,
                             void* stream) {
    PCC_REQUIRE(K >= 1 && K <= 27, "pcc_kernel_map_transpose: K out of range");
    PCC_REQUIRE(n_in < (1ll << 31) && n_out < (1ll << 31), "pcc_kernel_map_transpose: too many rows");
    hipStream_t st = as_stream(stream);
    if (n_in > 0) {
        PCC_CHECK_HIP(hipMemsetAsync(nbr_t, 0xFF, (size_t)n_in * K * sizeof(int32_t), st));
        PCC_CHECK_HIP(hipMemsetAsync(row_mask_t, 0, (size_t)n_in * sizeof(uint32_t), st));
    }
    if (n_out <= 0 || n_in <= 0) return PCC_OK;
    hipLaunchKernelGGL(map_transpose_kernel, dim3(blocks_for(n_out * K, 256)), dim3(256), 0, st, nbr, n_out, K, nbr_t, row_mask_t);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

static inline void launch_wgrad_reduce(const float* partial, int64_t elems, int nsplit, float* dw, hipStream_t st) {
    if (elems % 4 == 0 && ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(dw)) & 15) == 0)
        hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3(blocks_for(elems / 4, 256)), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(partial), elems / 4, nsplit, reinterpret_cast<float4*>(dw));
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks_for(elems, 256)), dim3(256), 0, st, partial, elems, nsplit, dw);
}
static inline bool wgrad_mfma(int cin, int cout) { return cin % 32 == 0 && cout % 32 == 0; }
static inline bool wgrad_rowsplit(int cin, int cout) { return wgrad_mfma(cin, cout) && cin <= 64 && cout <= 64; }
static inline int wgrad_splits(int64_t n_out) {            // at least ~48 row groups per workgroup
    const int64_t want = ((n_out + 31) / 32) / 48;
    return (int)(want < 8 ? 8 : (want > WG_SPLIT_MAX ? WG_SPLIT_MAX : want));
}
constexpr int WG_SPLIT_SLICE_MAX = 256;
static inline int wgrad_slice_splits(int64_t n_out) {      // three workgroup sets only: more splits to fill 256 CUs x 4
    const int64_t want = ((n_out + 31) / 32) / 24;
    return (int)(want < 8 ? 8 : (want > WG_SPLIT_SLICE_MAX ? WG_SPLIT_SLICE_MAX : want));
}

// ---------------------------------------------------------------------------------------------
// The plan of a weight-gradient launch: which kernel, how many row-group splits, how many partial images the second stage
// adds.  One place: the launches (pcc_conv_wgrad, pcc_conv_wgrad_bf16) and their names (pcc_conv_wgrad_kernel_name) follow it.
// The A/B switches are read once per process:
//   PCC_WGRAD_SLICE=0             keeps the one-offset kernel for 64-channel-class blocks of a 27-offset kernel (fp32)
//   PCC_WGRAD_SLICE_O=3|4|5|6|9   offsets per workgroup of the fp32 slice kernel (accumulators = 16 O registers per lane); 5
//   PCC_WGRAD_AHEAD=1|2           prefetch distance of its gathers; 2
//   PCC_WGRAD_BF16_SLICE_O=0|3|5|9  bf16 64 -> 64, 27 offsets: 0 keeps the one-offset kernel; 3.  850 k-row / 265 k-row shells,
//       same box: one-offset 122-124 / 129 TFLOP/s, O = 3 137 / 135 (71 registers, 7 waves per SIMD), O = 5 121 / 119 (103
//       registers), O = 9 140 / 125 (167 registers): fewer bytes and fewer waves trade evenly
// ---------------------------------------------------------------------------------------------
using SliceO = Choices<5, 3, 4, 6, 9>;          // PCC_WGRAD_SLICE_O
using SliceAhead = Choices<2, 1>;               // PCC_WGRAD_AHEAD
using Bf16SliceO = Choices<3, 0, 5, 9>;         // PCC_WGRAD_BF16_SLICE_O (0: the one-offset kernel)

static inline bool wgrad_slice_on() {
    static const bool on = [] { const char* e = getenv("PCC_WGRAD_SLICE"); return !(e && e[0] == '0'); }();
    return on;
}
static inline int wgrad_slice_o() { static const int O = SliceO::pick("PCC_WGRAD_SLICE_O"); return O; }
static inline int wgrad_ahead() { static const int ahead = SliceAhead::pick("PCC_WGRAD_AHEAD"); return ahead; }
static inline int wgrad_bf16_slice_o() { static const int O = Bf16SliceO::pick("PCC_WGRAD_BF16_SLICE_O"); return O; }

// Everything a launch needs, and its printed name
struct WgradPlan {
    void (*kernel)(WgradArgs);
    dim3 grid;
    size_t lds;           // dynamic LDS bytes
    int split;            // row-group splits (the thin kernel: WG_SPLIT_THIN row ranges)
    int partials;         // images [K][cin][cout] in the scratch
    char name[48];
};

// shape checks of a launch and its plan (n_out >= 1)
static int plan_wgrad(bool bf16, int K, int cin, int cout, int64_t n_out, WgradPlan& p) {
    // one offset and one block of up to 128 x 128 of W[k] per workgroup
    auto one_offset = [&](void (*kernel)(WgradArgs), const char* name, size_t lds, int per_split) {
        p.kernel = kernel;
        p.split = wgrad_splits(n_out);
        p.partials = p.split * per_split;
        p.grid = dim3((unsigned)(K * p.split), (unsigned)((cin + 127) / 128), (unsigned)((cout + 127) / 128));
        p.lds = lds;
        snprintf(p.name, sizeof p.name, "%s", name);
    };
    // O offsets per workgroup, dY rows staged once per group: 64-channel-class blocks of a 27-offset kernel
    auto slice = [&](void (*kernel)(WgradArgs), int O, size_t lds) {
        p.kernel = kernel;
        p.split = p.partials = wgrad_slice_splits(n_out);
        p.grid = dim3((unsigned)((K + O - 1) / O * p.split));
        p.lds = lds;
    };
    if (bf16) {
        PCC_REQUIRE(K >= 1 && K <= 27, "pcc_conv_wgrad_bf16: bad K");
        PCC_REQUIRE(cin % 64 == 0 && cout % 64 == 0 && cin >= 64 && cout >= 64, "pcc_conv_wgrad_bf16: cin and cout must be multiples of 64 (got %d, %d)", cin, cout);
        one_offset(conv_wgrad_bf16_kernel, "conv_wgrad_bf16_kernel", 4 * 2048 * sizeof(unsigned short), 1);
        if (cin == 64 && cout == 64 && K == 27)
            Bf16SliceO::dispatch(wgrad_bf16_slice_o(), [&](auto o) {
                constexpr int O = decltype(o)::value;
                if constexpr (O > 0) {
                    slice(conv_wgrad_bf16_slice_kernel<O>, O, (O + 1) * 2048 * sizeof(unsigned short));
                    snprintf(p.name, sizeof p.name, "conv_wgrad_bf16_slice_kernel<%d>", O);
                }
            });
        return PCC_OK;
    }
    PCC_REQUIRE(K >= 1 && K <= 27 && cin >= 1 && cout >= 1, "pcc_conv_wgrad: bad shape");
    if (!wgrad_mfma(cin, cout)) {
        PCC_REQUIRE((int64_t)cin * cout <= 4096, "pcc_conv_wgrad: thin path handles cin * cout <= 4096 (got %d x %d)", cin, cout);
        p.kernel = conv_wgrad_thin_kernel;
        p.split = p.partials = WG_SPLIT_THIN;
        p.grid = dim3((unsigned)(K * WG_SPLIT_THIN));
        p.lds = 0;
        snprintf(p.name, sizeof p.name, "conv_wgrad_thin_kernel");
    } else if (wgrad_slice_on() && wgrad_rowsplit(cin, cout) && K == 27) {
        SliceO::dispatch(wgrad_slice_o(), [&](auto o) {
            SliceAhead::dispatch(wgrad_ahead(), [&](auto ahead) {
                constexpr int O = decltype(o)::value, AHEAD = decltype(ahead)::value;
                slice(conv_wgrad_slice_kernel<O, AHEAD>, O, 2 * (AHEAD + 1) * 2048 * sizeof(float));
                snprintf(p.name, sizeof p.name, "conv_wgrad_slice_kernel<%d, %d>", O, AHEAD);
            });
        });
    } else {      // (64-channel class: two row groups per iteration, one partial per wave)
        one_offset(conv_wgrad_kernel, "conv_wgrad_kernel", 8 * 1024 * sizeof(float), wgrad_rowsplit(cin, cout) ? 4 : 1);
    }
    return PCC_OK;
}

int64_t pcc_conv_wgrad_scratch_elems(int32_t K, int32_t cin, int32_t cout) {
    // the largest layout any plan of the shape uses.  64-channel class: the one-offset kernel writes a partial per wave (4 per
    // split), the slice kernels one per split
    static_assert(WG_SPLIT_MAX * 4 >= WG_SPLIT_SLICE_MAX, "the rowsplit layout must bound the slice layout");
    const int partials = !wgrad_mfma(cin, cout) ? WG_SPLIT_THIN : WG_SPLIT_MAX * (wgrad_rowsplit(cin, cout) ? 4 : 1);
    return (int64_t)partials * K * cin * cout;
}

int pcc_conv_wgrad_kernel_name(int32_t bf16, int32_t K, int32_t cin, int32_t cout, int64_t n_out, char* buf, int32_t len,
                               int32_t* split, int32_t* partials) {
    WgradPlan p;
    if (int rc = plan_wgrad(bf16 != 0, K, cin, cout, n_out, p)) return rc;
    if (n_out <= 0) { p.split = p.partials = 0; p.name[0] = 0; }      // no kernel: the launch zero-fills dw
    if (split) *split = p.split;
    if (partials) *partials = p.partials;
    if (buf == nullptr) return PCC_OK;
    PCC_REQUIRE(snprintf(buf, len, "%s", p.name) < len, "pcc_conv_wgrad_kernel_name: %d bytes do not hold the name", len);
    return PCC_OK;
}

// The weight gradient of both entries: checks, plan, launch, reduce.  The fp32 entry looks at its shape, map and scratch (the
// bound of pcc_conv_wgrad_scratch_elems) first and at its operands only when there are rows and an MFMA kernel to run; the
// bf16 entry plans first, checks its operands whatever the row count, and bounds the scratch by what its plan writes.
// (bf16: fin and dy hold bf16, as in WgradArgs.)
static int wgrad(bool bf16, const float* fin, int64_t n_in, int cin, const float* dy, int64_t n_out, int cout, const int32_t* nbr,
                 const int32_t* order, const uint32_t* gmask, int K, float* dw, float* scratch, int64_t scratch_elems, void* stream) {
    const char* who = bf16 ? "pcc_conv_wgrad_bf16" : "pcc_conv_wgrad";
    const uint64_t esz = bf16 ? 2 : 4;
    WgradPlan p;
    auto check_operands = [&]() -> int {       // what the LDS-DMA kernels need of the gathered tensors
        PCC_REQUIRE((uint64_t)n_in * cin * esz <= BUF_OOB && (uint64_t)n_out * cout * esz <= BUF_OOB,
                    "%s: operands of 4 GiB and more are not supported", who);
        PCC_REQUIRE(((reinterpret_cast<uintptr_t>(fin) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0,
                    "%s: fin and dy must be 16-byte aligned (16-byte LDS-DMA loads)", who);
        return PCC_OK;
    };
    if (bf16) {
        if (int rc = plan_wgrad(true, K, cin, cout, n_out, p)) return rc;
        PCC_REQUIRE(nbr != nullptr, "%s: neighbour table required", who);
        if (int rc = check_operands()) return rc;
    } else {
        PCC_REQUIRE(K >= 1 && K <= 27 && cin >= 1 && cout >= 1, "%s: bad shape", who);
        PCC_REQUIRE(nbr != nullptr, "%s: neighbour table required (kernel_size 1: pass the identity map)", who);
        PCC_REQUIRE(scratch_elems >= pcc_conv_wgrad_scratch_elems(K, cin, cout), "%s: scratch too small", who);
    }
    hipStream_t st = as_stream(stream);
    const int64_t elems = (int64_t)K * cin * cout;
    if (n_out <= 0) {
        PCC_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)elems * sizeof(float), st));
        return PCC_OK;
    }
    if (bf16) {
        PCC_REQUIRE(scratch_elems >= (int64_t)p.partials * elems, "%s: scratch too small", who);
    } else {
        if (int rc = plan_wgrad(false, K, cin, cout, n_out, p)) return rc;
        if (p.kernel != conv_wgrad_thin_kernel)
            if (int rc = check_operands()) return rc;
    }
    const WgradArgs a = {fin, dy, nbr, order, gmask, scratch, n_in, n_out, cin, cout, K, p.split};
    hipLaunchKernelGGL(p.kernel, p.grid, dim3(256), p.lds, st, a);
    launch_wgrad_reduce(scratch, elems, p.partials, dw, st);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_conv_wgrad(const float* fin, int64_t n_in, int32_t cin, const float* dy, int64_t n_out, int32_t cout, const int32_t* nbr,
                   const int32_t* order, const uint32_t* group_mask32, int32_t K, float* dw, float* scratch, int64_t scratch_elems,
                   void* stream) {
    return wgrad(false, fin, n_in, cin, dy, n_out, cout, nbr, order, group_mask32, K, dw, scratch, scratch_elems, stream);
}

int pcc_conv_wgrad_bf16(const uint16_t* fin, int64_t n_in, int32_t cin, const uint16_t* dy, int64_t n_out, int32_t cout,
                        const int32_t* nbr, const int32_t* order, const uint32_t* group_mask32, int32_t K, float* dw, float* scratch,
                        int64_t scratch_elems, void* stream) {
    return wgrad(true, reinterpret_cast<const float*>(fin), n_in, cin, reinterpret_cast<const float*>(dy), n_out, cout, nbr, order,
                 group_mask32, K, dw, scratch, scratch_elems, stream);
}

}  // extern "C"
