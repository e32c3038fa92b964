// quality_batch.hpp — PSNR / SSIM of MANY views against as many references in one launch (lfi_compare_views; lfi_compare_view is n = 1): what the reference's
// scripts/compareDirs.sh gets from a loop of imageQualityMetrics.sh over two directories (reference scripts/compareDirs.sh,
// scripts/imageQualityMetrics.sh:1-12).  The definitions are include/lfi.h's, at lfi_compare_view (PSNR from the per-channel MSE over all pixels, SSIM = the mean
// over all 8×8 windows at stride 4 of the standard index with the window's biased moments); on top of them, exactly: the squared error per
// channel, the number of differing colour bytes and the largest difference.  Alpha is ignored.
//
//   quality_tiles<A_PLANAR, B_PLANAR>  grid = tiles in x × tiles in y × views, 256 lanes = 32 × 8 blocks of 4×4 pixels per step, up to
//     QB_STEPS steps down the tile.  Per step a lane loads its 4×4 block of both images — RGBA: four 16-byte loads each, transposed to one
//     dword per channel and row with v_perm; planar: one dword per colour plane and row, read as it is — the next step's loads are issued
//     before this step's arithmetic.  Per channel the block's moments Σa, Σb, Σa², Σb², Σab come from v_dot4_u32_u8 (four pixels per
//     instruction); the squared error is Σa² + Σb² − 2Σab, exact in integers.  The moments go to LDS as one 16-byte record per channel
//     (Σa and Σb share a dword); an 8×8 window is the sum of four blocks: the lane's own, its right neighbour and the two above them,
//     so a lane evaluates the window that ENDS in its block row — the row above is the previous step's last row, kept in a ring of three
//     groups of rows (one barrier per step).  The SSIM expression is the definition's, in fp64.  A tile owns 31 columns of windows and 63 rows:
//     neighbouring tiles overlap by one column and one row of blocks (the halo), whose pixels are counted by one of them only.
//     Lane sums → wave (shuffles) → workgroup (LDS, waves in order) → ONE QualityPartial per workgroup, stored: no atomics.
//   quality_views  one workgroup per view adds that view's partials: a lane its tiles in ascending order, then the same tree.  Every sum
//     has a fixed order: two calls on the same data give the same bits.
// Every partial and every per-view record is written by every call that reads it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace lfi {

constexpr int QB_LX = 32, QB_LY = 8;            // lanes of a workgroup, in blocks of 4×4 pixels
constexpr int QB_STEPS = 8;                     // steps of QB_LY block rows down a tile
constexpr int QB_TILE_BX = QB_LX - 1;           // block columns a tile owns (the 32nd is the right halo)
constexpr int QB_TILE_BY = QB_LY * QB_STEPS - 1; // block rows a tile owns (its first row is the halo of the tile above)

// Not a ViewsSrc (views_src.hpp): the references are host images or kept views with a stride of their own, and `pitch` is the bytes of a
// row in BOTH layouts (RGBA references come with the caller's pitch), where a ViewsSrc's is 0 for RGBA.
struct QualityImages
{
    const uint8_t *base; // image 0: RGBA rows of `pitch` bytes, or (planar) byte planes [R,G,B][H][pitch]
    size_t image_stride; // bytes from image to image
    uint32_t pitch;
};

struct QualityPartial // one per workgroup
{
    double ssim[3]; // Σ over the tile's windows
    unsigned long long sq_err[3];
    unsigned long long differing;
    uint32_t windows;
    uint32_t max_abs_diff;
};

struct QualityViewSums // one per view: what goes back to the host
{
    unsigned long long sq_err[3];
    unsigned long long differing;
    unsigned long long windows;
    double ssim[3]; // Σ over the view's windows
    int32_t max_abs_diff;
    int32_t reserved;
};

using qb_u32x4 = uint32_t __attribute__((ext_vector_type(4)));
using qb_i16x2 = short __attribute__((ext_vector_type(2)));
// a pixel row of an RGBA plane starts at a multiple of 4 bytes only (W·4 bytes per row, any W)
struct __attribute__((packed, aligned(4))) qb_px4
{
    qb_u32x4 v;
};

// byte i of the result = byte sel[i] of {hi, lo}: 0-3 from lo, 4-7 from hi (v_perm_b32)
__device__ inline uint32_t qb_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// the lane's 4×4 block at (x, y0) as one dword per row and channel: byte k = pixel x + k.  Pixels outside the image read as 0 in both
// images: they add nothing to any sum, difference or count.
template <bool PLANAR>
__device__ inline void qb_load(const uint8_t *img, const uint32_t pitch, const int W, const int H, const int x, const int y0, uint32_t (&out)[4][3])
{
#pragma unroll
    for(int r = 0; r < 4; r++)
    {
        const int y = y0 + r;
        out[r][0] = out[r][1] = out[r][2] = 0u;
        if(x < W && y < H)
        {
            if constexpr(PLANAR)
            {
                // x is a multiple of 4 below W: the dword lies inside the row's pitch (a multiple of 128); its bytes past W are padding
                const uint32_t mask = W - x >= 4 ? 0xffffffffu : (1u << (8 * (W - x))) - 1u;
#pragma unroll
                for(int ch = 0; ch < 3; ch++)
                    out[r][ch] = *reinterpret_cast<const uint32_t *>(img + ((size_t)ch * H + y) * pitch + x) & mask;
            }
            else
            {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(img + (size_t)y * pitch) + x;
                uint32_t p[4];
                if(x + 3 < W)
                {
                    const qb_u32x4 v = reinterpret_cast<const qb_px4 *>(src)->v;
                    p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
                }
                else
#pragma unroll
                    for(int k = 0; k < 4; k++)
                        p[k] = x + k < W ? src[k] : 0u;
                const uint32_t t0 = qb_perm(p[1], p[0], 0x05010400u), t1 = qb_perm(p[1], p[0], 0x06020602u); // R0 R1 G0 G1 / B0 B1 · ·
                const uint32_t u0 = qb_perm(p[3], p[2], 0x05010400u), u1 = qb_perm(p[3], p[2], 0x06020602u); // R2 R3 G2 G3 / B2 B3 · ·
                out[r][0] = qb_perm(u0, t0, 0x05040100u);
                out[r][1] = qb_perm(u0, t0, 0x07060302u);
                out[r][2] = qb_perm(u1, t1, 0x05040100u);
            }
        }
    }
}

__device__ inline double qb_ssim(const qb_u32x4 m)
{
    // m = {Σa | Σb << 16, Σa², Σb², Σab} over the window's 64 pixels; the definition's expression (include/lfi.h, lfi_compare_view)
    const uint32_t s1 = m.x & 0xffffu, s2 = m.x >> 16, s11 = m.y, s22 = m.z, s12 = m.w;
    const double C1 = 0.01 * 255.0 * 0.01 * 255.0, C2 = 0.03 * 255.0 * 0.03 * 255.0;
    const double mu1 = s1 / 64.0, mu2 = s2 / 64.0;
    const double var1 = s11 / 64.0 - mu1 * mu1, var2 = s22 / 64.0 - mu2 * mu2, cov = s12 / 64.0 - mu1 * mu2;
    return ((2.0 * mu1 * mu2 + C1) * (2.0 * cov + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (var1 + var2 + C2));
}

template <class T>
__device__ inline T qb_wave_sum(T v)
{
#pragma unroll
    for(int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    return v;
}

__device__ inline uint32_t qb_wave_max(uint32_t v)
{
#pragma unroll
    for(int off = 32; off > 0; off >>= 1)
        v = max(v, (uint32_t)__shfl_down(v, off));
    return v;
}

// a: the views (image blockIdx.z of a), b: their references (image blockIdx.z of b); partials: [gridDim.z][gridDim.y][gridDim.x]
template <bool A_PLANAR, bool B_PLANAR>
__global__ void __launch_bounds__(QB_LX *QB_LY) quality_tiles(const QualityImages a, const QualityImages b, const int W, const int H, QualityPartial *__restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) qb_u32x4 mom[3][3][QB_LY][QB_LX]; // [ring group][channel][block row][block column]
    __shared__ double red_ss[4][3];
    __shared__ uint32_t red_u[4][6];

    const int t = threadIdx.x, lx = t & (QB_LX - 1), ly = t / QB_LX;
    const int x = (blockIdx.x * QB_TILE_BX + lx) * 4;
    const int row0 = blockIdx.y * QB_TILE_BY; // the tile's first block row
    const int nby = (H + 3) / 4;
    const int nsteps = min(QB_STEPS, (nby - row0 + QB_LY - 1) / QB_LY); // ≥ 1: the launch has no tile below the image
    const uint8_t *img_a = a.base + (size_t)blockIdx.z * a.image_stride;
    const uint8_t *img_b = b.base + (size_t)blockIdx.z * b.image_stride;

    uint32_t se[3] = {0u, 0u, 0u}, differing = 0u, nwin = 0u;
    qb_i16x2 dmax = {0, 0}, dmin = {0, 0};
    double ss[3] = {0.0, 0.0, 0.0};

    uint32_t pa[4][3], pb[4][3];
    qb_load<A_PLANAR>(img_a, a.pitch, W, H, x, (row0 + ly) * 4, pa);
    qb_load<B_PLANAR>(img_b, b.pitch, W, H, x, (row0 + ly) * 4, pb);
    for(int s = 0; s < nsteps; s++)
    {
        const int br = row0 + s * QB_LY + ly; // this lane's block row
        uint32_t na[4][3], nb[4][3];          // the next step's block: in flight during this step's arithmetic
        if(s + 1 < nsteps)
        {
            qb_load<A_PLANAR>(img_a, a.pitch, W, H, x, (br + QB_LY) * 4, na);
            qb_load<B_PLANAR>(img_b, b.pitch, W, H, x, (br + QB_LY) * 4, nb);
        }
        // the halo is counted by the tile that owns it: the right column by the next tile, the first row by the tile above
        const bool not_right_halo = lx < QB_TILE_BX, not_top_halo = s > 0 || ly > 0; // the tile's 32nd column / its first block row
        const bool owned = not_right_halo && (not_top_halo || blockIdx.y == 0);
        qb_u32x4 m[3];
        const int g = s % 3;
#pragma unroll
        for(int c = 0; c < 3; c++)
        {
            uint32_t sa = 0u, sb = 0u, saa = 0u, sbb = 0u, sab = 0u, nz = 0u;
#pragma unroll
            for(int r = 0; r < 4; r++)
            {
                const uint32_t va = pa[r][c], vb = pb[r][c];
                sa = __builtin_amdgcn_udot4(va, 0x01010101u, sa, false);
                sb = __builtin_amdgcn_udot4(vb, 0x01010101u, sb, false);
                saa = __builtin_amdgcn_udot4(va, va, saa, false);
                sbb = __builtin_amdgcn_udot4(vb, vb, sbb, false);
                sab = __builtin_amdgcn_udot4(va, vb, sab, false);
                // bytes that differ: bit 7 of every non-zero byte of a ^ b
                const uint32_t d = va ^ vb;
                nz += __popc((((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u);
                // a − b per pixel, two pixels per packed 16-bit subtraction
                const qb_i16x2 de = __builtin_bit_cast(qb_i16x2, va & 0x00ff00ffu) - __builtin_bit_cast(qb_i16x2, vb & 0x00ff00ffu);
                const qb_i16x2 dodd = __builtin_bit_cast(qb_i16x2, (va >> 8) & 0x00ff00ffu) - __builtin_bit_cast(qb_i16x2, (vb >> 8) & 0x00ff00ffu);
                if(owned)
                {
                    dmax = __builtin_elementwise_max(dmax, __builtin_elementwise_max(de, dodd));
                    dmin = __builtin_elementwise_min(dmin, __builtin_elementwise_min(de, dodd));
                }
            }
            m[c] = qb_u32x4{sa | (sb << 16), saa, sbb, sab}; // Σa, Σb ≤ 16·255 per block and ≤ 64·255 per window: 16 bits each
            mom[g][c][ly][lx] = m[c];
            if(owned)
            {
                se[c] += saa + sbb - 2u * sab;
                differing += nz;
            }
        }
        __syncthreads();
        // the window whose lower left block is this lane's: blocks (br − 1, br) × (column, column + 1), if it lies inside the image
        if(not_right_halo && not_top_halo && x + 8 <= W && br * 4 + 4 <= H)
        {
            const int gu = ly > 0 ? g : (s + 2) % 3, ru = ly > 0 ? ly - 1 : QB_LY - 1; // the row above: the previous step's last row for ly == 0
#pragma unroll
            for(int c = 0; c < 3; c++)
                ss[c] += qb_ssim(m[c] + mom[g][c][ly][lx + 1] + mom[gu][c][ru][lx] + mom[gu][c][ru][lx + 1]);
            nwin++;
        }
        // no second barrier: the next step writes ring group (s + 1) % 3, which nobody reads now; group (s + 2) % 3 is written after the next barrier
        if(s + 1 < nsteps)
        {
#pragma unroll
            for(int r = 0; r < 4; r++)
#pragma unroll
                for(int c = 0; c < 3; c++)
                    pa[r][c] = na[r][c], pb[r][c] = nb[r][c];
        }
    }

    // lane → wave → workgroup, every sum in a fixed order
    const int hi = max(max((int)dmax.x, (int)dmax.y), max(-(int)dmin.x, -(int)dmin.y)); // ≥ 0: both start at 0
    const uint32_t wmax = qb_wave_max((uint32_t)hi);
    uint32_t wu[5] = {qb_wave_sum(se[0]), qb_wave_sum(se[1]), qb_wave_sum(se[2]), qb_wave_sum(differing), qb_wave_sum(nwin)};
    double wss[3] = {qb_wave_sum(ss[0]), qb_wave_sum(ss[1]), qb_wave_sum(ss[2])};
    const int wave = t >> 6;
    if((t & 63) == 0)
    {
#pragma unroll
        for(int c = 0; c < 3; c++)
            red_ss[wave][c] = wss[c];
#pragma unroll
        for(int k = 0; k < 5; k++)
            red_u[wave][k] = wu[k];
        red_u[wave][5] = wmax;
    }
    __syncthreads();
    if(t == 0)
    {
        QualityPartial p{};
        for(int w = 0; w < 4; w++)
        {
            for(int c = 0; c < 3; c++)
            {
                p.ssim[c] += red_ss[w][c];
                p.sq_err[c] += red_u[w][c];
            }
            p.differing += red_u[w][3];
            p.windows += red_u[w][4];
            p.max_abs_diff = max(p.max_abs_diff, red_u[w][5]);
        }
        partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
    }
}

// one workgroup per view: its `tiles` partials → one QualityViewSums
__global__ void __launch_bounds__(256) quality_views(const QualityPartial *__restrict__ partials, const int tiles, QualityViewSums *__restrict__ out)
{
    __shared__ double red_ss[4][3];
    __shared__ unsigned long long red_u[4][6];
    const int t = threadIdx.x;
    const QualityPartial *p = partials + (size_t)blockIdx.x * tiles;
    double ss[3] = {0.0, 0.0, 0.0};
    unsigned long long u[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    uint32_t mx = 0u;
    for(int i = t; i < tiles; i += 256)
    {
#pragma unroll
        for(int c = 0; c < 3; c++)
        {
            ss[c] += p[i].ssim[c];
            u[c] += p[i].sq_err[c];
        }
        u[3] += p[i].differing;
        u[4] += p[i].windows;
        mx = max(mx, p[i].max_abs_diff);
    }
#pragma unroll
    for(int c = 0; c < 3; c++)
        ss[c] = qb_wave_sum(ss[c]);
#pragma unroll
    for(int k = 0; k < 5; k++)
        u[k] = qb_wave_sum(u[k]);
    mx = qb_wave_max(mx);
    const int wave = t >> 6;
    if((t & 63) == 0)
    {
#pragma unroll
        for(int c = 0; c < 3; c++)
            red_ss[wave][c] = ss[c];
#pragma unroll
        for(int k = 0; k < 5; k++)
            red_u[wave][k] = u[k];
        red_u[wave][5] = mx;
    }
    __syncthreads();
    if(t == 0)
    {
        QualityViewSums v{};
        unsigned long long m = 0ull;
        for(int w = 0; w < 4; w++)
        {
            for(int c = 0; c < 3; c++)
            {
                v.ssim[c] += red_ss[w][c];
                v.sq_err[c] += red_u[w][c];
            }
            v.differing += red_u[w][3];
            v.windows += red_u[w][4];
            m = max(m, red_u[w][5]);
        }
        v.max_abs_diff = (int32_t)m;
        out[blockIdx.x] = v;
    }
}

inline int quality_tiles_x(const int W) { return ((W + 3) / 4 + QB_TILE_BX - 1) / QB_TILE_BX; }
// a tile owns block rows (row0, row0 + 63], the first tile row 0 as well
inline int quality_tiles_y(const int H) { return std::max(1, ((H + 3) / 4 - 1 + QB_TILE_BY - 1) / QB_TILE_BY); }

// Enqueues ONE quality_tiles launch for n views and their n references; partials: n · tiles_x · tiles_y records.
inline hipError_t launch_quality_tiles(hipStream_t stream, const bool a_planar, const bool b_planar, const QualityImages &a, const QualityImages &b, const int W,
                                       const int H, const int n, QualityPartial *partials)
{
    const dim3 grid(quality_tiles_x(W), quality_tiles_y(H), n), block(QB_LX * QB_LY);
    if(a_planar && b_planar)
        hipLaunchKernelGGL((quality_tiles<true, true>), grid, block, 0, stream, a, b, W, H, partials);
    else if(a_planar)
        hipLaunchKernelGGL((quality_tiles<true, false>), grid, block, 0, stream, a, b, W, H, partials);
    else if(!b_planar)
        hipLaunchKernelGGL((quality_tiles<false, false>), grid, block, 0, stream, a, b, W, H, partials);
    else
        return hipErrorInvalidValue; // RGBA views against planar references: kept views share the views' layout
    return hipGetLastError();
}

} // namespace lfi
