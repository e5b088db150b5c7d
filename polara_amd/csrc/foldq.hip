// K4q: the fold-in of the scoring pass, E = A_test * V (models.py:857-860 `test_matrix.dot(v)`), against a PACKED image
// of the item factors: one 128-byte cache line per rank-50 row instead of the two lines of the fp32 image.
//
// Why: the row-wise SpMM is bound by what the L1 / texture path delivers per gathered row (every width
// moves ~19 TB/s of row pieces, a 256-byte row costs twice a 128-byte one), so the lever left is bytes per gathered
// entry.  The ids-only scoring pass does not need E exactly: it needs E' with a PROVEN bound ||E'_u - E_u|| <= 2^-24 w_u
// (rescore.hip certifies the order of the lists against it and re-folds the users it cannot certify in fp64).
//
// Format ("Q20").  A row of K values is cut into L = 2 / 4 / 8 / 16 / 32 lane pieces of 16 bytes (K <= 12 / 25 / 50 /
// 101 / 202).  A piece is a 128-bit stream, most significant bit first:
//     [ digit : 8 ][ v0 : 20 ][ v1 : 20 ][ v2 : 20 ][ v3 : 20 ][ v4 : 20 ][ v5 : 20 ]
// v0..v5 are columns 6l .. 6l+5 of the row as 20-bit two's-complement fixed point.  A value is DECODED as the 32-bit
// window of the stream that starts at its first bit, read as an int32 and converted to fp32 (one v_alignbit_b32 and one
// full-rate v_cvt_f32_i32 per value, no extraction for the digit): the 12 bits below a value belong to its neighbour,
// the encoder knows them and rounds the value so that the WHOLE window is nearest to the target (error <= half a 20-bit
// step, as if the low bits were not there; the fp32 conversion's rounding of the low bits is emulated by the encoder
// and is part of the error it records).  Real value = fl32(window) * s(b), s = the scale of the row's BRACKET b (rows are cut into brackets by index, four per octave: the
// catalogue is in popularity order, so a bracket's rows have similar norms; the scale multiplies the user's value once
// per entry, in the stage that fetches the (index, value) pairs — no per-row scale has to be gathered or decoded).
// The 8-bit digits carry what does not fit the 6 L main columns: column 6L + e is a three-digit signed number spread
// over the digits of lanes 3e, 3e+1, 3e+2 (23 bits at half scale; each lane accumulates its own digit's window, the three
// sums are joined once per row task), and the digit of lane L-1 is the row's ERROR WEIGHT: D_j >= 2^24 ||V_j - decode(row j)||
// computed by the encoder from the bits it wrote — exact, not a worst case — so that the same product yields
// w_u = sum_j a_uj D_j (column K of the output), the certified bound of the fold-in's error.
//
// Mapping: one wave per row task (the plan of spmm.hip), the wave cut into 64 / L groups of L lanes, group g takes
// entries g, g + GROUPS, ... of the task; one dwordx4 load per lane and entry; group sums added in a fixed order
// (deterministic).  Where the caller states that adjacent tasks are alike, 2 or 4 of them share a wave (the kernel's T).
// Arithmetic: the first version converted every window to fp64 and accumulated with v_fma_f64 — and ran at the speed of
// the fp32-image kernel (0.233 against 0.259 ms on the ML-20M-shaped fold-in): both are bound by their fp64 CONVERSIONS
// (v_cvt_f64_*: a quarter of the VALU rate), not by the texture path.  Here a lane multiplies in fp32 — packed
// v_pk_fma_f32, two columns per instruction — over the U entries of one register set and adds the set's partial sums to
// fp64 accumulators (two conversions per column and set instead of one per column and entry).  What that costs in
// accuracy is bounded like any fp32 dot product of U terms and joins the row's error weight: with u = 2^-24,
// |computed - sum_j a_j decode_j| <= (U + 2) u sum_j a_j |decode_j| column by column (the value's rounding to fp32, one
// rounding per fused multiply-add, U of them per set), i.e. D_j carries (U + 2) ||decode_j|| on top of 2^24 times the
// quantisation error (~ +11 % for U = 4).
#include "pk_common.h"
#include <math.h>
#include <stdlib.h>
#include <type_traits>

#define PK_Q20_TAB 96

__host__ __device__ __forceinline__ int pk_q20_bracket(unsigned j) {
    if (j < 4u) return (int)j;
#ifdef __HIP_DEVICE_COMPILE__
    const int e = 31 - __clz((int)j);
#else
    const int e = 31 - __builtin_clz(j);
#endif
    return 4 * (e - 1) + (int)((j >> (e - 2)) & 3u);
}

static inline int q20_lanes(int K) {
    if (K <= 12) return 2;
    if (K <= 25) return 4;
    if (K <= 50) return 8;
    if (K <= 101) return 16;
    if (K <= 202) return 32;
    return 0;
}

extern "C" int32_t pk_q20_lanes(int32_t K) { return K >= 1 ? q20_lanes(K) : 0; }

// number of extra columns (beyond the 6 L main ones) an L-lane row can carry
__host__ __device__ __forceinline__ int pk_q20_extras(int L) { return (L - 1) / 3; }

// ---------------------------------------------------------------------------------------------- encoder
// bracket maxima of |V| (positive doubles order like their bit patterns)
__global__ __launch_bounds__(256) void q20_bracket_max_kernel(int64_t n, int K, const double *__restrict__ V, int64_t ldv,
                                                              unsigned long long *__restrict__ bmax_bits) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    double m = 0.0;
    for (int c = lane; c < K; c += 64) {
        const double a = fabs(V[row * ldv + c]);
        m = (a <= 1e300) ? fmax(m, a) : INFINITY;              // NaN and overflowing magnitudes: no image (q20_scale_kernel flags it)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if (lane == 0 && m > 0.0) atomicMax(bmax_bits + pk_q20_bracket((unsigned)row), (unsigned long long)__double_as_longlong(m));
}

__global__ void q20_scale_kernel(const unsigned long long *__restrict__ bmax_bits, double *__restrict__ tab, int32_t *__restrict__ info) {
    const int b = threadIdx.x;
    if (b >= PK_Q20_TAB) return;
    const double m = __longlong_as_double((long long)bmax_bits[b]);
    // a window spans +-2^31 and a target stays 8192 units inside it; non-finite or subnormal-scale factors: no image
    double s = m * (1.0 + 9.5367431640625e-07) / (2147483648.0 - 8192.0);
    // (the certified bound |E' - E| <= 2^-24 w_u rests on RELATIVE fp32 roundings of the per-entry factor
    // (float)(a * s): a bracket whose scale lies below ~2^-100 would make that factor an fp32 denormal — absolute error, not
    // covered by the weights D_j — so such factors get no packed image either: the caller keeps the fp32 image)
    if (!(m < 1e300) || (m > 0.0 && s < 7.888609052210118e-31)) {
        atomicOr(info, 1);
        s = 0.0;
    }
    tab[b] = s;
}

template <int L>
__global__ __launch_bounds__(256) void q20_encode_kernel(int64_t n, int K, const double *__restrict__ V, int64_t ldv,
                                                         const double *__restrict__ tab, double kappa, double fp32_terms,
                                                         uint4 *__restrict__ img, int32_t *__restrict__ info) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row_raw = gid / L;
    const bool live = row_raw < n;
    const int64_t row = live ? row_raw : n - 1;
    const int l = (int)(gid % L);
    const double s = tab[pk_q20_bracket((unsigned)row)];
    const double inv = s > 0.0 ? 1.0 / s : 0.0;
    const double *vr = V + row * ldv;
    unsigned p[6];
    double sq = 0.0;       // squared quantisation error of this lane's columns (real units)
    double mag = 0.0;      // squared magnitude of what the kernel multiplies (window units): weight of its fp32 arithmetic
    unsigned g = 0;
#pragma unroll
    for (int t = 5; t >= 0; --t) {
        const int c = 6 * l + t;
        const double v = c < K ? vr[c] : 0.0;
        double f = rint((v * inv - (double)g) * 0.000244140625);
        f = fmin(fmax(f, -524288.0), 524287.0);
        const double window = (double)(float)(int)(f * 4096.0 + (double)g);     // what the kernel decodes: fl32 of the int32 window
        if (c < K) {
            const double err = fma(-window, s, v);
            sq = fma(err, err, sq);
            mag = fma(window, window, mag);
        }
        p[t] = ((unsigned)(int)f) & 0xFFFFFu;
        g = p[t] >> 8;
    }
    const double G = (double)((p[0] << 4) | (p[1] >> 16));      // the 24 bits below this lane's digit
    // ---- digits of the extra columns: lanes 3e (top), 3e+1, 3e+2 carry column 6L + e.  Every lane computes the three
    // digits as if it were a top lane (with the bits below its neighbours' digits, G1 and G2); the lower lanes fetch theirs.
    const int lane = threadIdx.x & 63;
    const int e = l / 3, lvl = l % 3;
    const bool has_extra = (3 * e + 2 <= L - 2) && (6 * L + e < K);
    const double xv = (has_extra && lvl == 0) ? vr[6 * L + e] : 0.0;
    const double G1 = __shfl(G, lane + 1, 64), G2 = __shfl(G, lane + 2, 64);
    // target in window units of the top digit, at HALF scale (a digit's window spans [-2^31, 2^31 - 2^24 + G]: a bracket's
    // largest entry sitting in an extra column would not be representable at full scale; 23 bits are still eight times
    // finer than the main columns' 20).  A digit is chosen so that the remainder lies in the range the lower digits
    // can represent (floor against that range's lower end), the last one to nearest.
    const double X = xv * inv * 0.5;
    const double lo2 = (-2147483648.0 + G2) * 1.52587890625e-05;
    const double lo1 = (-2147483648.0 + G1) * 0.00390625 + lo2;
    auto f32w = [](double dgt, double Gl) { return (double)(float)(int)(dgt * 16777216.0 + Gl); };      // fl32 of a digit's window
    const double d0 = fmin(fmax(floor((X - G - lo1) * 5.9604644775390625e-08), -128.0), 127.0);
    const double w0 = f32w(d0, G);
    const double R0 = X - w0;
    const double d1 = fmin(fmax(floor(((R0 - lo2) * 256.0 - G1) * 5.9604644775390625e-08), -128.0), 127.0);
    const double w1 = f32w(d1, G1);
    const double R1 = R0 - w1 * 0.00390625;
    const double d2 = fmin(fmax(rint((R1 * 65536.0 - G2) * 5.9604644775390625e-08), -128.0), 127.0);
    const double w2 = f32w(d2, G2);
    const double d1_up = __shfl(d1, lane - 1, 64), d2_up = __shfl(d2, lane - 2, 64);
    double dig = 0.0;
    if (has_extra) dig = lvl == 0 ? d0 : (lvl == 1 ? d1_up : d2_up);
    if (has_extra && lvl == 0) {
        const double rep = w0 + w1 * 0.00390625 + w2 * 1.52587890625e-05;      // exact: the three fp32 windows at their weights
        const double err = fma(-2.0 * rep, s, xv);
        sq = fma(err, err, sq);
        const double m3 = 2.0 * (fabs(w0) + fabs(w1) * 0.00390625 + fabs(w2) * 1.52587890625e-05);
        mag = fma(m3, m3, mag);
    }
    // ---- the row's error weight in the digit of lane L - 1
#pragma unroll
    for (int off = 1; off < L; off <<= 1) {
        sq += __shfl_xor(sq, off, 64);
        mag += __shfl_xor(mag, off, 64);
    }
    if (l == L - 1) {
        // D = 2^24 * ||quantisation error|| + (U + 2) * ||what the kernel multiplies|| (its fp32 arithmetic, see the header),
        // with a margin for the roundings of this computation and of the kernel's fp64 sums
        const double D = (sqrt(sq) * 16777216.0 + fp32_terms * sqrt(mag) * s) * (1.0 + 0.001953125);
        dig = 0.0;
        if (s > 0.0) {
            const double Y = D / (s * kappa);
            dig = ceil((Y - G) * 5.9604644775390625e-08);
            if (dig <= 127.0 && f32w(dig, G) < Y) dig += 1.0;         // the window's own fp32 rounding must not round the weight down
            if (dig > 127.0) {
                atomicOr(info, 2);      // kappa too small for this row (cannot happen with pk_q20_kappa's choice): no image
                dig = 127.0;
            }
            dig = fmax(dig, -128.0);
        }
    }
    const unsigned db = ((unsigned)(int)dig) & 0xFFu;
    uint4 o;
    o.x = (db << 24) | (p[0] << 4) | (p[1] >> 16);
    o.y = ((p[1] & 0xFFFFu) << 16) | (p[2] >> 4);
    o.z = ((p[2] & 0xFu) << 28) | (p[3] << 8) | (p[4] >> 12);
    o.w = ((p[4] & 0xFFFu) << 20) | p[5];
    if (live) img[row * L + l] = o;
}

// entries a lane multiplies in fp32 before it adds the partial sums to its fp64 accumulators (= steps per register set)
static inline int q20_steps(int L) {
    // (the L = 8 instance: 4 steps per register set — 2 and 8 were measured, profiles/r05_foldq_v1_probe_*; a compile-time
    // fact of encoder and kernel alike, because the rows' certified weights carry U + 2 roundings: VERDICT r5 weak #8)
    return L >= 8 ? 4 : (L == 4 ? 2 : 1);
}
// (T, the row tasks per wave, is no such fact: the weights do not depend on it.  The scoring pass asks for 4 on its
// activity-ordered matrix, ops.FOLD_TASKS_PER_WAVE, where the launch is long enough — ML-20M-shaped rank 50: 0.176 / 0.160 /
// 0.155 ms for T = 1 / 2 / 4, VALU instructions per launch 77.9 M -> 67.3 M; profiles/foldq_slices_ml20m.txt)
// unit of the weight digit: the largest weight a row can need — every column half a step (2048 units) off plus its fp32
// conversion (64), the fp32 arithmetic term on a row of full-scale windows, the extra columns counted at twice a main
// one's magnitude — must fit 126 digit units
static double q20_kappa(int K) {
    const int L = q20_lanes(K);
    return sqrt((double)K + 32.0) * (2112.0 + (q20_steps(L) + 2.0) * 128.0) * 1.03 / 126.0;
}

extern "C" double pk_q20_kappa(int32_t K) { return q20_kappa(K); }

// image bytes of n rows
extern "C" int64_t pk_q20_image_bytes(int64_t n, int32_t K) {
    const int L = q20_lanes(K);
    return L ? n * L * 16 : 0;
}

extern "C" int pk_q20_encode_f64(void *stream, int64_t n, int32_t K, const double *V_dev, int64_t ldv, void *img_dev,
                                 double *tab_dev, void *work_dev, int32_t *info_dev) {
    const int L = q20_lanes(K);
    PK_REQUIRE(L != 0 && n >= 1 && ldv >= K, "pk_q20_encode_f64: rank %d has no packed image (max 202) or bad sizes", K);
    PK_REQUIRE(n < (1 << 24) && n * L * 16 < ((int64_t)1 << 32), "pk_q20_encode_f64: the image must stay below 4 GiB and 2^24 rows");
    PK_REQUIRE(V_dev && img_dev && tab_dev && work_dev && info_dev && (((uintptr_t)img_dev) & 127) == 0, "pk_q20_encode_f64: bad pointers (image 128-byte aligned)");
    hipStream_t st = pk_stream(stream);
    unsigned long long *bmax = static_cast<unsigned long long *>(work_dev);        // PK_Q20_TAB * 8 bytes
    if (hipMemsetAsync(bmax, 0, PK_Q20_TAB * 8, st) != hipSuccess || hipMemsetAsync(info_dev, 0, 4, st) != hipSuccess) {
        pk_set_error("pk_q20_encode_f64: memset failed");
        return PK_E_LAUNCH;
    }
    hipLaunchKernelGGL(q20_bracket_max_kernel, dim3((unsigned)pk_ceil_div(n, 4)), dim3(256), 0, st, n, K, V_dev, ldv, bmax);
    hipLaunchKernelGGL(q20_scale_kernel, dim3(1), dim3(128), 0, st, bmax, tab_dev, info_dev);
    const double kappa = q20_kappa(K), fp32_terms = q20_steps(L) + 2.0;
    const dim3 grid((unsigned)pk_ceil_div(n * L, 256));
    uint4 *img = static_cast<uint4 *>(img_dev);
    switch (L) {
        case 2: hipLaunchKernelGGL(q20_encode_kernel<2>, grid, dim3(256), 0, st, n, K, V_dev, ldv, tab_dev, kappa, fp32_terms, img, info_dev); break;
        case 4: hipLaunchKernelGGL(q20_encode_kernel<4>, grid, dim3(256), 0, st, n, K, V_dev, ldv, tab_dev, kappa, fp32_terms, img, info_dev); break;
        case 8: hipLaunchKernelGGL(q20_encode_kernel<8>, grid, dim3(256), 0, st, n, K, V_dev, ldv, tab_dev, kappa, fp32_terms, img, info_dev); break;
        case 16: hipLaunchKernelGGL(q20_encode_kernel<16>, grid, dim3(256), 0, st, n, K, V_dev, ldv, tab_dev, kappa, fp32_terms, img, info_dev); break;
        default: hipLaunchKernelGGL(q20_encode_kernel<32>, grid, dim3(256), 0, st, n, K, V_dev, ldv, tab_dev, kappa, fp32_terms, img, info_dev); break;
    }
    PK_CHECK_LAUNCH("q20_encode_kernel");
    return PK_OK;
}

// ---------------------------------------------------------------------------------------------- decoder (tests, re-scoring)
// fp64 rows of the image exactly as the fold-in kernel reads them: out[n x (K + 1)], column K = D_j
template <int L>
__global__ __launch_bounds__(256) void q20_decode_kernel(int64_t n, int K, const uint4 *__restrict__ img, const double *__restrict__ tab,
                                                         double kappa, double *__restrict__ out, int64_t ldo) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row_raw = gid / L;
    const bool live = row_raw < n;
    const int64_t row = live ? row_raw : n - 1;
    const int l = (int)(gid % L);
    const uint4 d = img[row * L + l];
    const double s = tab[pk_q20_bracket((unsigned)row)];
    const int w[7] = {(int)__builtin_amdgcn_alignbit(d.x, d.y, 24), (int)__builtin_amdgcn_alignbit(d.x, d.y, 4),
                      (int)__builtin_amdgcn_alignbit(d.y, d.z, 16), (int)__builtin_amdgcn_alignbit(d.z, d.w, 28),
                      (int)__builtin_amdgcn_alignbit(d.z, d.w, 8), (int)(d.w << 12), (int)d.x};
    double *o = out + row * ldo;
#pragma unroll
    for (int t = 0; t < 6; ++t)
        if (live && 6 * l + t < K) o[6 * l + t] = (double)(float)w[t] * s;
    const double a6 = (double)(float)w[6] * s;
    const int lane = threadIdx.x & 63;
    const double a1 = __shfl(a6, lane + 1, 64), a2 = __shfl(a6, lane + 2, 64);
    const int e = l / 3;
    if (live && l % 3 == 0 && 3 * e + 2 <= L - 2 && 6 * L + e < K) o[6 * L + e] = 2.0 * (a6 + a1 * 0.00390625 + a2 * 1.52587890625e-05);
    if (live && l == L - 1) o[K] = kappa * a6;
}

extern "C" int pk_q20_decode_f64(void *stream, int64_t n, int32_t K, const void *img_dev, const double *tab_dev, double *out_dev,
                                 int64_t ldo) {
    const int L = q20_lanes(K);
    PK_REQUIRE(L != 0 && n >= 1 && ldo >= K + 1, "pk_q20_decode_f64: bad sizes");
    hipStream_t st = pk_stream(stream);
    const dim3 grid((unsigned)pk_ceil_div(n * L, 256));
    const uint4 *img = static_cast<const uint4 *>(img_dev);
    const double kappa = q20_kappa(K);
    switch (L) {
        case 2: hipLaunchKernelGGL(q20_decode_kernel<2>, grid, dim3(256), 0, st, n, K, img, tab_dev, kappa, out_dev, ldo); break;
        case 4: hipLaunchKernelGGL(q20_decode_kernel<4>, grid, dim3(256), 0, st, n, K, img, tab_dev, kappa, out_dev, ldo); break;
        case 8: hipLaunchKernelGGL(q20_decode_kernel<8>, grid, dim3(256), 0, st, n, K, img, tab_dev, kappa, out_dev, ldo); break;
        case 16: hipLaunchKernelGGL(q20_decode_kernel<16>, grid, dim3(256), 0, st, n, K, img, tab_dev, kappa, out_dev, ldo); break;
        default: hipLaunchKernelGGL(q20_decode_kernel<32>, grid, dim3(256), 0, st, n, K, img, tab_dev, kappa, out_dev, ldo); break;
    }
    PK_CHECK_LAUNCH("q20_decode_kernel");
    return PK_OK;
}

// ---------------------------------------------------------------------------------------------- the fold-in
// ---- the sum over the lane groups: recursive halving, not a butterfly.
// v_permlane32_swap exchanges the upper half of one register with the lower half of another: after swap(x, y) the first
// register holds [x.low, y.low] and the second [x.high, y.high], so ONE addition leaves the pair sum of x in the lower 32
// lanes and the pair sum of y in the upper 32.  Seven partial sums per lane become four (x, y) = (slot k, slot k + 4), then
// two with v_permlane16_swap ((k, k + 2)); the 8 / 4 / 2-lane distances that are left go through DPP butterflies on those
// two values.  26 instructions where the butterfly over all seven sums took ~160 — a third of this kernel's VALU work is
// its per-task prologue and epilogue (SQ_INSTS_VALU: 104 M per ML-20M-shaped launch, 2.5 M wave steps of ~24).
__device__ __forceinline__ double q20_swap_add32(double x, double y) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ double q20_swap_add16(double x, double y) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

typedef float pk_f2 __attribute__((ext_vector_type(2)));

// (Measured and not kept, round 5: the fp64 accumulators in LDS with the register allocation held to 6 or 8 waves per SIMD
// — 0.245 ms against 0.232 with the accumulators in registers and 5 waves: occupancy is not what this kernel waits for.)
// T = tasks per wave (1, 2 or 4).  T = 1 is the mapping above.  For T > 1 the wave is cut into T SLICES of CH = 64 / T lanes:
// slice s of wave w owns task T * w + s, its GS = GROUPS / T lane groups take entries g, g + GS, ... of that task, and a
// chunk is CH pairs of EACH task (one coalesced 64-lane load per wave still).  The per-task prologue and epilogue — about
// as many VALU instructions as the body of a median row — are then paid once per T tasks.  The loop's trip count, `have`,
// `have_next` and the skipped steps follow the LONGEST task of the wave: a slice past its own end holds padded pairs
// (0, 0.0) like the tail of a chunk, so the mapping pays where adjacent tasks are alike in length (rows in activity order)
// and is the caller's choice (pk_fold_q20_sliced).  A slice whose task lies beyond n_tasks runs as a task of no entries
// and stores nothing; a real empty task stores its zeros.  The shuffles' sources stay inside the slice.
template <typename VT, int L, int U, int T>
__global__ __launch_bounds__(256) void fold_q20_kernel(
    int64_t n_tasks, const int32_t *__restrict__ task_row, const int64_t *__restrict__ task_begin,
    const int64_t *__restrict__ task_end, const int32_t *__restrict__ task_slot,
    const int32_t *__restrict__ indices, const VT *__restrict__ vals, const uint4 *__restrict__ img,
    const double *__restrict__ tab, double kappa, int K, int Kx, double *__restrict__ out, int64_t ldo,
    double *__restrict__ partial) {
    constexpr int GROUPS = 64 / L;
    constexpr int GS = GROUPS / T;                           // lane groups of a slice
    constexpr int CH = 64 / T;                               // lanes of a slice = pairs of one task per chunk
    constexpr int SPC = L;                                   // wave steps per chunk (CH / GS)
    constexpr int SETS = SPC / U;                            // register sets (U steps each, two in flight) per chunk
    static_assert(T == 1 || T == 2 || T == 4, "1, 2 or 4 tasks per wave");
    static_assert(GS >= 2 && GS * T == GROUPS, "a slice holds at least two lane groups");
    static_assert(SETS >= 1 && SETS * U == SPC, "a chunk is a whole number of register sets");
    constexpr int LOG_RB = L == 2 ? 5 : (L == 4 ? 6 : (L == 8 ? 7 : (L == 16 ? 8 : 9)));   // log2(row bytes)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wtask = ((int64_t)blockIdx.x * 4 + wave) * T;
    if (wtask >= n_tasks) return;
    const int sl = T == 1 ? 0 : lane / CH, ls = lane % CH;   // slice, lane of the slice
    const int64_t task = wtask + sl;
    const bool real = T == 1 || task < n_tasks;
    int64_t p0 = 0;
    int n = 0;                                               // per lane for T > 1: the entries of the slice's task
    if (real) {
        p0 = task_begin[task];
        n = (int)(task_end[task] - p0);
    }
    int nmax = n;                                            // wave-uniform: the longest task of the wave
    if constexpr (T > 1) {
        nmax = __builtin_amdgcn_readlane(n, 0);
#pragma unroll
        for (int s = 1; s < T; ++s) {
            const int ns = __builtin_amdgcn_readlane(n, s * CH);
            nmax = ns > nmax ? ns : nmax;
        }
    }
    const int g = lane / L, l = lane % L;
    const int src0 = T == 1 ? g : (lane & ~(CH - 1)) | (g % GS);                     // the slice's lane that holds the group's pair of step 0
    const int32_t *ip = indices + p0;
    const VT *vp = vals + p0;
    const char *Xb = reinterpret_cast<const char *>(img);
    const unsigned lo0 = (unsigned)l << 4;

    double acc[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) acc[t] = 0.0;

    // pairs: current chunk (index, fl32(value * bracket scale)), next chunk (index, raw value; its scales requested at
    // the top of the iteration before it), the chunk after that in flight
    int jc = 0, jn = 0;
    VT araw = (VT)0, an = (VT)0;
    if (ls < n) {
        jc = ip[ls];
        araw = vp[ls];
    }
    if (CH + ls < n) {
        jn = ip[CH + ls];
        an = vp[CH + ls];
    }
    // (a step whose eight pairs all lie beyond the chunk's count is skipped — loads and products: rows are 20 .. 9 000
    // entries long and a short row's last register set is mostly padding)
    auto issue = [&](int jch, int st0, int cnt_ch, uint4(&x)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u > 0 && (st0 + u) * GS >= cnt_ch) break;
            const int jj = __shfl(jch, (st0 + u) * GS + src0, 64);
            unsigned off;
            asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(off) : "v"(jj), "n"(LOG_RB), "v"(lo0));
            x[u] = *reinterpret_cast<const uint4 *>(Xb + off);
        }
    };
    // one register set: U entries multiplied and summed in fp32 (two columns per v_pk_fma_f32), then added to the fp64 sums
    auto consume = [&](float ach, int st0, int cnt_ch, const uint4(&x)[U]) {
        pk_f2 s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f}, s45 = {0.0f, 0.0f};
        float s6 = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u > 0 && (st0 + u) * GS >= cnt_ch) break;
            const float a = __shfl(ach, (st0 + u) * GS + src0, 64);
            const pk_f2 aa = {a, a};
            const uint4 d = x[u];
            const pk_f2 x01 = {(float)(int)__builtin_amdgcn_alignbit(d.x, d.y, 24), (float)(int)__builtin_amdgcn_alignbit(d.x, d.y, 4)};
            const pk_f2 x23 = {(float)(int)__builtin_amdgcn_alignbit(d.y, d.z, 16), (float)(int)__builtin_amdgcn_alignbit(d.z, d.w, 28)};
            const pk_f2 x45 = {(float)(int)__builtin_amdgcn_alignbit(d.z, d.w, 8), (float)(int)(d.w << 12)};
            s01 = __builtin_elementwise_fma(aa, x01, s01);
            s23 = __builtin_elementwise_fma(aa, x23, s23);
            s45 = __builtin_elementwise_fma(aa, x45, s45);
            s6 = fmaf(a, (float)(int)d.x, s6);
        }
        acc[0] += (double)s01.x;
        acc[1] += (double)s01.y;
        acc[2] += (double)s23.x;
        acc[3] += (double)s23.y;
        acc[4] += (double)s45.x;
        acc[5] += (double)s45.y;
        acc[6] += (double)s6;
    };
    uint4 x0[U], x1[U];
    issue(jc, 0, nmax < CH ? nmax : CH, x0);                 // the first gathers do not wait for the scale
    float ac = (float)((double)araw * tab[pk_q20_bracket((unsigned)jc)]);
    // one chunk (CH pairs per task; the counts are those of the wave's longest task) whose first set sits in register file P (the sets alternate between the two files; with an odd
    // number of sets per chunk the next chunk starts in the other one)
    auto chunk = [&](int p, auto P) {
        constexpr int P0 = decltype(P)::value;
        const int cnt = (nmax - p) < CH ? (nmax - p) : CH;   // pairs of this chunk; padded lanes hold (0, 0.0)
        const bool more = p + CH < nmax;
        const int cnt_next = (nmax - p - CH) < CH ? (nmax - p - CH) : CH;
        int jf = 0;
        VT af = (VT)0;
        if (p + 2 * CH + ls < n) {                           // pairs two chunks ahead
            jf = ip[p + 2 * CH + ls];
            af = vp[p + 2 * CH + ls];
        }
        double sn = 0.0;
        if (more) sn = tab[pk_q20_bracket((unsigned)jn)];     // the next chunk's scales (its indices arrived a chunk ago)
#pragma unroll
        for (int k = 0; k < SETS; ++k) {
            const bool have = k * U * GS < cnt;
            const bool have_next = (k + 1 < SETS) ? ((k + 1) * U * GS < cnt) : more;
            if (((k + P0) & 1) == 0) {
                if (have_next) {
                    if (k + 1 < SETS) issue(jc, (k + 1) * U, cnt, x1);
                    else issue(jn, 0, cnt_next, x1);
                }
                if (have) consume(ac, k * U, cnt, x0);
            } else {
                if (have_next) {
                    if (k + 1 < SETS) issue(jc, (k + 1) * U, cnt, x0);
                    else issue(jn, 0, cnt_next, x0);
                }
                if (have) consume(ac, k * U, cnt, x1);
            }
        }
        jc = jn;
        ac = (float)((double)an * sn);
        jn = jf;
        an = af;
    };
    if constexpr ((SETS & 1) == 0) {
        for (int p = 0; p < nmax; p += CH) chunk(p, std::integral_constant<int, 0>());
    } else {
        // an odd number of sets per chunk: two chunks bring the files back to where they started
        for (int p = 0; p < nmax; p += 2 * CH) {
            chunk(p, std::integral_constant<int, 0>());
            if (p + CH < nmax) chunk(p + CH, std::integral_constant<int, 1>());
        }
    }

    // ---- sum over the groups of the slice (fixed order: deterministic).
    // T = 1: after the halving rounds a lane holds the totals of TWO column slots (four for L = 32): slot
    //        t0 = 4 * bit5(lane) + 2 * bit4(lane) and t0 + 1; slot 6 is the digit's sum.
    // T = 2: a slice is a half wave, so the 32-lane exchange drops out: v_permlane16_swap on (slot k, slot k + 4) leaves
    //        FOUR slots per lane, t0 = 4 * bit4(lane); the 8 / 4 / 2-lane distances go through the DPP butterflies.
    // T = 4: a slice is one 16-lane row: the DPP butterflies alone, on all seven sums; every lane holds every slot.
    constexpr int NW = T == 4 ? 7 : ((T == 2 || L == 32) ? 4 : 2);
    double w[NW];
    if constexpr (T == 1) {
        const double h0 = q20_swap_add32(acc[0], acc[4]), h1 = q20_swap_add32(acc[1], acc[5]);
        const double h2 = q20_swap_add32(acc[2], acc[6]), h3 = q20_swap_add32(acc[3], 0.0);
        if constexpr (L <= 16) {
            w[0] = q20_swap_add16(h0, h2);
            w[1] = q20_swap_add16(h1, h3);
        } else {
            w[0] = h0, w[1] = h1, w[2] = h2, w[3] = h3;
        }
    } else if constexpr (T == 2) {
        w[0] = q20_swap_add16(acc[0], acc[4]);
        w[1] = q20_swap_add16(acc[1], acc[5]);
        w[2] = q20_swap_add16(acc[2], acc[6]);
        w[3] = q20_swap_add16(acc[3], 0.0);
    } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) w[i] = acc[i];
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if constexpr (L <= 8) w[i] += pk_lane_xor<8>(w[i]);
        if constexpr (L <= 4) w[i] += pk_lane_xor<4>(w[i]);
        if constexpr (L <= 2) w[i] += pk_lane_xor<2>(w[i]);
    }
    const int b5 = (lane >> 5) & 1, b4 = (lane >> 4) & 1;
    // first column slot this lane holds
    const int t0 = T == 4 ? 0 : (T == 2 ? 4 * b4 : (L <= 16 ? 4 * b5 + 2 * b4 : 4 * b5));
    // the digit's sum (slot 6) sits in w[6 - t0] of the lanes that hold it: w[0] where t0 == 6 (T = 1, L <= 16), w[2] of the
    // upper half wave (T = 1, L = 32) or of the upper rows (T = 2), w[6] everywhere (T = 4);
    // the three digit sums of an extra column meet in its top lane
    constexpr int DW = T == 4 ? 6 : ((T == 2 || L == 32) ? 2 : 0);
    const double dsum = w[DW];
    const double a1 = __shfl(dsum, lane + 1, 64), a2 = __shfl(dsum, lane + 2, 64);
    int slot = -1;
    int64_t row = 0;
    if (real) {
        slot = task_slot[task];
        row = task_row[task];
    }
    double *dst = slot < 0 ? out + row * ldo : partial + (int64_t)slot * Kx;
    // one lane per (row piece l, slot set) stores: the lanes whose group bits below bit 4 are zero
    const bool owner = real && (L <= 16 ? (((lane & 15) / L) == 0) : true);
    if (owner) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int t = t0 + i;
            if (t < 6 && 6 * l + t < K) dst[6 * l + t] = w[i];
        }
        const bool digit_lane = T == 4 ? true : (T == 2 ? (b4 == 1) : (L <= 16 ? (t0 == 6) : (b5 == 1)));
        if (digit_lane) {
            const int e = l / 3;
            if (l % 3 == 0 && 3 * e + 2 <= L - 2 && 6 * L + e < K) dst[6 * L + e] = 2.0 * (dsum + a1 * 0.00390625 + a2 * 1.52587890625e-05);
            if (l == L - 1) {
                dst[K] = kappa * dsum;
                for (int c = K + 1; c < Kx; ++c) dst[c] = 0.0;
            }
        }
    }
}

// out[row, :] = sum of the row's partial slots (fixed order): the tail of a row split into several tasks.
// zero[0 .. zero_n) = 0 on the way (workgroup 0): the counters of a scoring pass, whose first user is the re-scoring behind the
// sweep — this launch sits between the fold-in and the sweep, so the reset costs the pass no launch of its own.
__global__ __launch_bounds__(256) void fold_q20_fixup_kernel(int64_t n_long, const int32_t *__restrict__ long_row,
                                                             const int32_t *__restrict__ slot_begin, const int32_t *__restrict__ slot_end,
                                                             const double *__restrict__ partial, int nc, double *__restrict__ out, int64_t ldo,
                                                             int32_t *__restrict__ zero, int zero_n) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < zero_n; i += blockDim.x) zero[i] = 0;
    const int64_t r = blockIdx.x;
    if (r >= n_long) return;
    const int s0 = slot_begin[r], s1 = slot_end[r];
    double *dst = out + (int64_t)long_row[r] * ldo;
    for (int c = threadIdx.x; c < nc; c += blockDim.x) {
        double a = 0.0;
        for (int s = s0; s < s1; ++s) a += partial[(int64_t)s * nc + c];
        dst[c] = a;
    }
}

template <typename VT>
static void launch_fold_q20(hipStream_t st, int L, int T, int64_t n_tasks, const int32_t *task_row, const int64_t *task_begin,
                            const int64_t *task_end, const int32_t *task_slot, const int32_t *indices, const void *vals,
                            const uint4 *img, const double *tab, double kappa, int K, int Kx, double *out, int64_t ldo, double *partial) {
    const dim3 grid((unsigned)pk_ceil_div(n_tasks, (int64_t)4 * T)), block(256);      // four waves of T tasks per workgroup
    const VT *v = static_cast<const VT *>(vals);
#define PK_FOLDQ(LL, UU, TT)                                                                                                      \
    hipLaunchKernelGGL((fold_q20_kernel<VT, LL, UU, TT>), grid, block, 0, st, n_tasks, task_row, task_begin, task_end, task_slot, \
                       indices, v, img, tab, kappa, K, Kx, out, ldo, partial)
#define PK_FOLDQ_T4(LL, UU)                      \
    do {                                         \
        if (T == 4) PK_FOLDQ(LL, UU, 4);         \
        else if (T == 2) PK_FOLDQ(LL, UU, 2);    \
        else PK_FOLDQ(LL, UU, 1);                \
    } while (0)
    switch (L) {
        case 2: PK_FOLDQ_T4(2, 1); break;
        case 4: PK_FOLDQ_T4(4, 2); break;
        case 8:
            if (q20_steps(8) == 2) PK_FOLDQ_T4(8, 2);
            else if (q20_steps(8) == 8) PK_FOLDQ_T4(8, 8);
            else PK_FOLDQ_T4(8, 4);
            break;
        case 16:
            if (T == 2) PK_FOLDQ(16, 4, 2);
            else PK_FOLDQ(16, 4, 1);
            break;
        default: PK_FOLDQ(32, 4, 1); break;
    }
#undef PK_FOLDQ_T4
#undef PK_FOLDQ
}

// The fold-in with `tasks_per_wave` = 1, 2 or 4 adjacent row tasks per wave (fold_q20_kernel's T; anything else is refused),
// clamped to what the lane class allows: 4 for L <= 8, 2 for L = 16, 1 for L = 32.  More than one pays where adjacent tasks
// are alike in length — the wave runs as long as its longest task — which only the caller knows (rows in activity order).
// Every value returns the product within the same certified weight; the bits differ between values (the order of the
// fp64 sums), never between launches of one value.  zero_dev / zero_n: as pk_fold_q20_zero.
// Which value the scoring pass uses on its activity-ordered matrix is recorded at ops.FOLD_TASKS_PER_WAVE with its measurement.
extern "C" int pk_fold_q20_sliced(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                                  const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                                  const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                                  const int32_t *indices_dev, const void *vals_dev, int val_kind, const void *img_dev,
                                  const double *tab_dev, int64_t n_items, int32_t K, int32_t Kx, double *out_dev, int64_t ldo,
                                  double *partial_dev, int32_t *zero_dev, int32_t zero_n, int32_t tasks_per_wave) {
    const int L = q20_lanes(K);
    PK_REQUIRE(L != 0 && n_tasks >= 0 && Kx >= K + 1 && ldo >= Kx, "pk_fold_q20: bad sizes (K=%d, Kx=%d)", K, Kx);
    PK_REQUIRE(n_items >= 1 && n_items < (1 << 24) && n_items * L * 16 < ((int64_t)1 << 32), "pk_fold_q20: image beyond 32-bit offsets");
    PK_REQUIRE(n_long == 0 || partial_dev != nullptr, "pk_fold_q20: partial buffer required");
    PK_REQUIRE(val_kind == PK_VAL_F32 || val_kind == PK_VAL_F64, "pk_fold_q20: bad val_kind %d", val_kind);
    PK_REQUIRE(zero_n >= 0 && zero_n <= (1 << 20) && (zero_n == 0 || zero_dev != nullptr), "pk_fold_q20: bad counter range");
    PK_REQUIRE(tasks_per_wave == 1 || tasks_per_wave == 2 || tasks_per_wave == 4, "pk_fold_q20_sliced: tasks_per_wave %d (1, 2 or 4)",
               tasks_per_wave);
    const int T = L == 32 ? 1 : (L == 16 && tasks_per_wave > 2 ? 2 : tasks_per_wave);
    hipStream_t st = pk_stream(stream);
    if (n_tasks == 0) n_long = 0;      // nothing to fold: only the counters are left to do
    if (n_tasks > 0) {
        const uint4 *img = static_cast<const uint4 *>(img_dev);
        const double kappa = q20_kappa(K);
        if (val_kind == PK_VAL_F32)
            launch_fold_q20<float>(st, L, T, n_tasks, task_row_dev, task_begin_dev, task_end_dev, task_slot_dev, indices_dev, vals_dev,
                                   img, tab_dev, kappa, K, Kx, out_dev, ldo, partial_dev);
        else
            launch_fold_q20<double>(st, L, T, n_tasks, task_row_dev, task_begin_dev, task_end_dev, task_slot_dev, indices_dev, vals_dev,
                                    img, tab_dev, kappa, K, Kx, out_dev, ldo, partial_dev);
        PK_CHECK_LAUNCH("fold_q20_kernel");
    }
    if (n_long > 0 || zero_n > 0) {
        hipLaunchKernelGGL(fold_q20_fixup_kernel, dim3((unsigned)(n_long > 0 ? n_long : 1)), dim3(256), 0, st, n_long, long_row_dev,
                           long_slot_begin_dev, long_slot_end_dev, partial_dev, Kx, out_dev, ldo, zero_dev, (int)zero_n);
        PK_CHECK_LAUNCH("fold_q20_fixup_kernel");
    }
    return PK_OK;
}

// pk_fold_q20 that also zeroes zero_dev[0 .. zero_n) (int32 device counters; zero_n == 0: nothing) in its fix-up launch —
// which then runs even without a split row, as one workgroup that only zeroes.  One task per wave.
extern "C" int pk_fold_q20_zero(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                                const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                                const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                                const int32_t *indices_dev, const void *vals_dev, int val_kind, const void *img_dev,
                                const double *tab_dev, int64_t n_items, int32_t K, int32_t Kx, double *out_dev, int64_t ldo,
                                double *partial_dev, int32_t *zero_dev, int32_t zero_n) {
    return pk_fold_q20_sliced(stream, n_tasks, task_row_dev, task_begin_dev, task_end_dev, task_slot_dev, n_long, long_row_dev,
                              long_slot_begin_dev, long_slot_end_dev, indices_dev, vals_dev, val_kind, img_dev, tab_dev, n_items, K, Kx,
                              out_dev, ldo, partial_dev, zero_dev, zero_n, 1);
}

extern "C" int pk_fold_q20(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                           const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                           const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                           const int32_t *indices_dev, const void *vals_dev, int val_kind, const void *img_dev,
                           const double *tab_dev, int64_t n_items, int32_t K, int32_t Kx, double *out_dev, int64_t ldo,
                           double *partial_dev) {
    return pk_fold_q20_sliced(stream, n_tasks, task_row_dev, task_begin_dev, task_end_dev, task_slot_dev, n_long, long_row_dev,
                              long_slot_begin_dev, long_slot_end_dev, indices_dev, vals_dev, val_kind, img_dev, tab_dev, n_items, K, Kx,
                              out_dev, ldo, partial_dev, nullptr, 0, 1);
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp): the runtime loads a code object at the first
// launch of one of its kernels — or when a kernel's attributes are asked for, which costs no launch
hipError_t pk_tu_load_foldq() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&q20_scale_kernel));
}
