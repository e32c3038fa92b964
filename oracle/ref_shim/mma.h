/* mma.h — nvcuda::wmma as far as the reference's src/kernels.cu uses it: the m32n8k16 shape with half operands and a half
 * accumulator.  TEST INFRASTRUCTURE ONLY; every line is this project's (see ref_cuda.h).
 *
 * The calls are collective over the 32 consecutive linear thread ids of a warp.  CUDA leaves a fragment's distribution over the
 * lanes unspecified; here lane r holds row r of matrix_a and of the accumulator, and every lane holds all of matrix_b.  A load
 * or store synchronises the warp before it (the other lanes' writes to shared memory are done) and after it (nobody overwrites
 * what a lane has yet to read).
 *
 * ASSUMPTION (the one thing here that no source text defines): mma_sync with a half accumulator is modelled exactly as the
 * oracle's M16 (oracle/lfi_oracle.c, lfo_blend_ten): per call acc = fp16_rn(acc + Σ₁₆ a·b), the sum of the 16 products
 * exact and ONE rounding to nearest even.  With the kernels' operands (bytes × fp16 weights, both multiples of 2^-24 below
 * 2^16) the products and their sum are exact in double.  What this pins is everything around the instruction; the
 * hardware's accumulate rounding stays a model.
 */
#ifndef REF_SHIM_MMA_H
#define REF_SHIM_MMA_H

#include "cuda_fp16.h"

namespace nvcuda
{
namespace wmma
{
struct matrix_a;
struct matrix_b;
struct accumulator;
struct row_major;
struct col_major;
enum layout_t { mem_row_major, mem_col_major };

template <typename Use, int M, int N, int K, typename T, typename Layout = void>
struct fragment;

/* M×K, row-major source: lane r holds row r */
template <int M, int N, int K>
struct fragment<matrix_a, M, N, K, half, row_major>
{
    static_assert(M == 32 && N == 8 && K == 16, "only m32n8k16 is used");
    half row[K];
};

/* K×N, column-major source: every lane holds the whole matrix, element (k, n) at [n][k] */
template <int M, int N, int K>
struct fragment<matrix_b, M, N, K, half, col_major>
{
    static_assert(M == 32 && N == 8 && K == 16, "only m32n8k16 is used");
    half col[N][K];
};

/* M×N: lane r holds row r */
template <int M, int N, int K>
struct fragment<accumulator, M, N, K, half, void>
{
    static_assert(M == 32 && N == 8 && K == 16, "only m32n8k16 is used");
    half row[N];
};

template <int M, int N, int K>
inline void fill_fragment(fragment<accumulator, M, N, K, half> &f, half value)
{
    for(int n = 0; n < N; n++)
        f.row[n] = value;
}

/* "ldm describes the stride in elements between consecutive rows (for row major layout) or columns (for column major layout)" */
template <int M, int N, int K>
inline void load_matrix_sync(fragment<matrix_a, M, N, K, half, row_major> &f, const half *p, unsigned ldm)
{
    ref_shim::syncWarp();
    const int r = ref_shim::lane();
    for(int k = 0; k < K; k++)
        f.row[k] = p[static_cast<size_t>(r) * ldm + k];
    ref_shim::syncWarp();
}

template <int M, int N, int K>
inline void load_matrix_sync(fragment<matrix_b, M, N, K, half, col_major> &f, const half *p, unsigned ldm)
{
    ref_shim::syncWarp();
    for(int n = 0; n < N; n++)
        for(int k = 0; k < K; k++)
            f.col[n][k] = p[static_cast<size_t>(n) * ldm + k];
    ref_shim::syncWarp();
}

/* double → half in ONE rounding to nearest even, done by hand: a compiler may lower the conversion through float, which
 * rounds twice.  The double is scaled so that one unit is the half's last place, rounded there, and scaled back; the result
 * is a half's value, so the conversions that follow are exact. */
inline half roundToHalf(double d)
{
    double a = std::fabs(d);
    if(!(a < 65520.0)) /* halfway between the largest finite half and 2^16 rounds to infinity; NaN stays NaN */
        return half(static_cast<float>(std::isnan(d) ? d : std::copysign(HUGE_VAL, d)));
    int e = 0;
    (void)std::frexp(a, &e);
    e = e - 1 < -14 ? -14 : e - 1; /* a in [2^e, 2^(e+1)), subnormals share the exponent -14 */
    double q = std::nearbyint(std::ldexp(a, 10 - e));
    return half(static_cast<float>(std::copysign(std::ldexp(q, e - 10), d)));
}

/* d = a·b + c, see ASSUMPTION above */
template <int M, int N, int K>
inline void mma_sync(fragment<accumulator, M, N, K, half> &d, const fragment<matrix_a, M, N, K, half, row_major> &a,
                     const fragment<matrix_b, M, N, K, half, col_major> &b, const fragment<accumulator, M, N, K, half> &c)
{
    for(int n = 0; n < N; n++)
    {
        double sum = 0.0;
        for(int k = 0; k < K; k++)
            sum += static_cast<double>(static_cast<float>(a.row[k])) * static_cast<double>(static_cast<float>(b.col[n][k]));
        d.row[n] = roundToHalf(static_cast<double>(static_cast<float>(c.row[n])) + sum);
    }
}

template <int M, int N, int K>
inline void store_matrix_sync(half *p, const fragment<accumulator, M, N, K, half> &f, unsigned ldm, layout_t layout)
{
    if(layout != mem_row_major)
        ref_shim::trap("store_matrix_sync: only mem_row_major is used by the kernels", 0, 0, 0);
    ref_shim::syncWarp();
    const int r = ref_shim::lane();
    for(int n = 0; n < N; n++)
        p[static_cast<size_t>(r) * ldm + n] = f.row[n];
    ref_shim::syncWarp();
}
} // namespace wmma
} // namespace nvcuda

#endif
