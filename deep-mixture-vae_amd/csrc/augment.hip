// Random affine warp of rows on the device: every row of X [n_rows][ldx] (f32) is a single-plane H x W image, row-major, and out [n_rows][ldo] gets
// its warp under the row's own SAMPLING map theta = (m00 m01 m02 | m10 m11 m12), in pixel-index units, from output pixel to source coordinate:
//   output pixel (row i, column j):   sx = fmaf(m00, j, fmaf(m01, i, m02)),   sy = fmaf(m10, j, fmaf(m11, i, m12))          (float32, this order)
//   x0 = floor(sx), fx = sx - x0 (exact), y0, fy alike; the four taps v00 = S(y0, x0), v01 = S(y0, x0 + 1), v10 = S(y0 + 1, x0), v11 = S(y0 + 1, x0 + 1)
//   of the source image EXTENDED BY ZEROS (a tap outside [0, W) x [0, H) is 0);
//   top = fmaf(fx, v01 - v00, v00),  bot = fmaf(fx, v11 - v10, v10),  out = fmaf(fy, bot - top, top).
// That is grid_sample(mode = bilinear, padding_mode = zeros, align_corners = True) after the unit conversion.  A coordinate that is NaN, Inf or
// outside (-1, W) x (-1, H) gives 0 (every tap lies outside).  Integer maps (identity, shifts, flips, quarter turns) give fx = fy = 0 and copy
// the tap's bits (a -0 comes out as +0).
//   the draw (theta_in null): uniforms of Philox stream 9 at (seed, step = counter), blocks 2 g and 2 g + 1, g = row_base + r the row's index in
//   the UNPERMUTED data set; u = (w >> 8) * 2^-24, s = 2 u - 1 (exact).  Block 2 g: angle = rotate_deg s0, tx = translate_px s1, ty = translate_px s2,
//   scale = expf(fmaf(u3, log hi - log lo, log lo)); block 2 g + 1: shear = shear_deg s0 (words 1 .. 3 reserved).  Forward transform about the
//   centre c = ((W - 1) / 2, (H - 1) / 2):  p_out = c + t + scale R(angle) Shear_x(tan shear) (p_in - c);  theta is its inverse in closed form,
//     k = tanf(shear), (sn, cs) = sincosf(angle), inv = 1 / scale:   m00 = fmaf(k, sn, cs) inv, m01 = fmaf(-k, cs, sn) inv, m10 = -sn inv, m11 = cs inv,
//     q = c + t:   m02 = fmaf(-m01, qy, fmaf(-m00, qx, cx)),  m12 = fmaf(-m11, qy, fmaf(-m10, qx, cy)).
//   Zero ranges with scale (1, 1) give exactly (1 0 0 | 0 1 0) up to the sign of a zero: out == X in bits.
//   augment_rows_kernel  256 threads.  An image of at most 1024 pixels belongs to ONE WAVE (four images per block), a larger one to the block; the
//                        block walks the images by a stride that is the same for all of its waves, so the two barriers of a round are met by
//                        every thread (a wave past the last row idles through them).  The image is staged in LDS as it lies in memory (H W
//                        floats, never padded: 16 KiB at most, one fixed 16 KiB array) with 16-byte loads where the row's address allows, scalar
//                        loads otherwise; the first lane of the image's group forms the six coefficients once and shares them through LDS (and
//                        writes theta_out).  Each lane then produces runs of four consecutive output pixels and stores 16 bytes where the
//                        address allows; taps outside the image are predicated (their index is clamped and the value replaced by 0).  Pad
//                        columns of out are never written.  No atomics, no inter-block dependence, no scratch: 8 bytes per element.
#include "augment.h"

#include <cmath>

namespace dmvae {

struct AugmentArgs {
    const float* X; int64_t ldx;
    float* out; int64_t ldo;
    const float* theta_in; float* theta_out;
    int64_t n_rows; uint64_t row_base;
    int H, W, HW, ipb;                            // ipb: images per block, 4 (a wave each) or 1
    uint64_t seed, counter;
    float rotate_deg, translate_px, shear_deg, log_lo, log_span;
};

constexpr int AUGMENT_WAVE_PIXELS = 1024;        // the largest image a single wave takes: four of them fill the 16 KiB

__device__ __forceinline__ float augment_sym(uint32_t w) {       // s = 2 u - 1 in [-1, 1), exact
    return fmaf(2.0f, (float)(w >> 8) * (1.0f / 16777216.0f), -1.0f);
}

__device__ __forceinline__ void augment_draw(const AugmentArgs& a, uint64_t g, float (&m)[6]) {
    uint32_t w0[4], w1[4];
    philox_block(a.seed, a.counter, AUGMENT_PHILOX_STREAM, 2 * g, w0);
    philox_block(a.seed, a.counter, AUGMENT_PHILOX_STREAM, 2 * g + 1, w1);
    const float DEG = 0.017453292519943295f;
    const float angle = (a.rotate_deg * augment_sym(w0[0])) * DEG;
    const float tx = a.translate_px * augment_sym(w0[1]), ty = a.translate_px * augment_sym(w0[2]);
    const float scale = expf(fmaf((float)(w0[3] >> 8) * (1.0f / 16777216.0f), a.log_span, a.log_lo));
    const float k = tanf((a.shear_deg * augment_sym(w1[0])) * DEG);
    float sn, cs;
    sincosf(angle, &sn, &cs);
    const float inv = 1.0f / scale;
    const float cx = 0.5f * (float)(a.W - 1), cy = 0.5f * (float)(a.H - 1);
    const float qx = cx + tx, qy = cy + ty;
    m[0] = fmaf(k, sn, cs) * inv;
    m[1] = fmaf(-k, cs, sn) * inv;
    m[3] = -sn * inv;
    m[4] = cs * inv;
    m[2] = fmaf(-m[1], qy, fmaf(-m[0], qx, cx));
    m[5] = fmaf(-m[4], qy, fmaf(-m[3], qx, cy));
}

__device__ __forceinline__ float augment_sample(const float* im, int W, int H, float fW, float fH, const float (&m)[6], int i, int j) {
    const float fi = (float)i, fj = (float)j;
    const float sx = fmaf(m[0], fj, fmaf(m[1], fi, m[2]));
    const float sy = fmaf(m[3], fj, fmaf(m[4], fi, m[5]));
    if (!(sx > -1.0f && sx < fW && sy > -1.0f && sy < fH)) return 0.0f;          // NaN, Inf, or every tap outside
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                                       // in [-1, W - 1] and [-1, H - 1]
    const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
    const int c0 = xl ? x0 : 0, c1 = xr ? x0 + 1 : W - 1;
    const int r0 = (yt ? y0 : 0) * W, r1 = (yb ? y0 + 1 : H - 1) * W;
    const float t00 = im[r0 + c0], t01 = im[r0 + c1], t10 = im[r1 + c0], t11 = im[r1 + c1];
    const float v00 = (xl && yt) ? t00 : 0.0f, v01 = (xr && yt) ? t01 : 0.0f;
    const float v10 = (xl && yb) ? t10 : 0.0f, v11 = (xr && yb) ? t11 : 0.0f;
    const float top = fmaf(fx, v01 - v00, v00);
    const float bot = fmaf(fx, v11 - v10, v10);
    return fmaf(fy, bot - top, top);
}

__global__ __launch_bounds__(256) void augment_rows_kernel(AugmentArgs a) {
    __shared__ __attribute__((aligned(16))) float img[4 * AUGMENT_WAVE_PIXELS];
    __shared__ float coef[4][8];
    const int tpi = 256 / a.ipb;                                  // threads per image: 64 or 256
    const int slot = (int)threadIdx.x / tpi, lt = (int)threadIdx.x - slot * tpi;
    float* im = img + slot * AUGMENT_WAVE_PIXELS;                 // (one image per block: slot 0, the whole array)
    const float fW = (float)a.W, fH = (float)a.H;
    const int64_t stride = (int64_t)gridDim.x * a.ipb;
    for (int64_t base = (int64_t)blockIdx.x * a.ipb; base < a.n_rows; base += stride) {      // the same trip count for every thread of the block
        const int64_t r = base + slot;
        const bool live = r < a.n_rows;
        if (live) {
            const float* x = a.X + r * a.ldx;
            if (((uintptr_t)x & 15) == 0) {
                const int nq = a.HW >> 2;
                for (int q = lt; q < nq; q += tpi) reinterpret_cast<f32x4*>(im)[q] = reinterpret_cast<const f32x4*>(x)[q];
                for (int e = 4 * nq + lt; e < a.HW; e += tpi) im[e] = x[e];
            } else {
                for (int e = lt; e < a.HW; e += tpi) im[e] = x[e];
            }
            if (lt == 0) {
                float m[6];
                if (a.theta_in) {
#pragma unroll
                    for (int e = 0; e < 6; ++e) m[e] = a.theta_in[r * 6 + e];
                } else {
                    augment_draw(a, a.row_base + (uint64_t)r, m);
                }
#pragma unroll
                for (int e = 0; e < 6; ++e) coef[slot][e] = m[e];
                if (a.theta_out) {
#pragma unroll
                    for (int e = 0; e < 6; ++e) a.theta_out[r * 6 + e] = m[e];
                }
            }
        }
        __syncthreads();
        if (live) {
            float m[6];
#pragma unroll
            for (int e = 0; e < 6; ++e) m[e] = coef[slot][e];
            float* o = a.out + r * a.ldo;
            const bool aligned = ((uintptr_t)o & 15) == 0;
            const int nruns = (a.HW + 3) >> 2;
            for (int q = lt; q < nruns; q += tpi) {
                const int p0 = 4 * q;
                int i = p0 / a.W, j = p0 - i * a.W;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {                     // (past the image's last pixel, in the last run: computed on clamped taps, not stored)
                    v[e] = augment_sample(im, a.W, a.H, fW, fH, m, i, j);
                    if (++j == a.W) { j = 0; ++i; }
                }
                if (p0 + 4 <= a.HW) {
                    if (aligned) {
                        const f32x4 y = {v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(o + p0) = y;
                    } else {
                        o[p0] = v[0]; o[p0 + 1] = v[1]; o[p0 + 2] = v[2]; o[p0 + 3] = v[3];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (p0 + e < a.HW) o[p0 + e] = v[e];
                }
            }
        }
        __syncthreads();                                          // the next round overwrites the image and the coefficients
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define AUGMENT_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int augment_rows_launch(hipStream_t s, const float* X, int64_t ldx, int64_t n_rows, int H, int W, int64_t row_base, uint64_t seed, uint64_t counter,
                        const dmvae_augment_params* p, const float* theta_in, float* theta_out, float* out, int64_t ldo) {
    const char* who = "dmvae_augment_rows";
    AUGMENT_REQUIRE(X && out, "%s: null X / out", who);
    AUGMENT_REQUIRE(p || theta_in, "%s: null params without theta_in (the draw needs its ranges)", who);
    AUGMENT_REQUIRE(n_rows >= 1, "%s: n_rows=%lld (n_rows >= 1)", who, (long long)n_rows);
    AUGMENT_REQUIRE(H >= 1 && W >= 1 && H <= AUGMENT_MAX_SIDE && W <= AUGMENT_MAX_SIDE, "%s: H=%d, W=%d (1 <= H, W <= %d: an image is staged in 16 KiB of LDS)", who,
                    H, W, AUGMENT_MAX_SIDE);
    const int HW = H * W;
    AUGMENT_REQUIRE(ldx >= HW && ldo >= HW, "%s: ldx=%lld, ldo=%lld (ldx >= H W, ldo >= H W = %d)", who, (long long)ldx, (long long)ldo, HW);
    AUGMENT_REQUIRE(row_base >= 0, "%s: row_base=%lld (row_base >= 0)", who, (long long)row_base);
    typedef unsigned __int128 u128;
    AUGMENT_REQUIRE(2 * ((u128)row_base + (u128)n_rows) < (u128)AUGMENT_MAX_BLOCK, "%s: 2 (row_base + n_rows) = 2 (%lld + %lld) reaches 2^56: the block index would "
                    "enter the stream bits", who, (long long)row_base, (long long)n_rows);
    float log_lo = 0.0f, log_span = 0.0f;
    if (!theta_in) {
        AUGMENT_REQUIRE(std::isfinite(p->rotate_deg) && p->rotate_deg >= 0.0f && std::isfinite(p->translate_px) && p->translate_px >= 0.0f &&
                        std::isfinite(p->shear_deg) && p->shear_deg >= 0.0f, "%s: rotate_deg=%g, translate_px=%g, shear_deg=%g (ranges are finite and >= 0)", who,
                        (double)p->rotate_deg, (double)p->translate_px, (double)p->shear_deg);
        AUGMENT_REQUIRE(std::isfinite(p->scale_lo) && std::isfinite(p->scale_hi) && p->scale_lo > 0.0f && p->scale_lo <= p->scale_hi,
                        "%s: scale_lo=%g, scale_hi=%g (finite, 0 < scale_lo <= scale_hi)", who, (double)p->scale_lo, (double)p->scale_hi);
        log_lo = (float)std::log((double)p->scale_lo);
        log_span = (float)std::log((double)p->scale_hi) - log_lo;
    }
    // the byte spans of the two sides, first element to last; a span past the address space cannot be a buffer
    const u128 xb = (u128)(uintptr_t)X, ob = (u128)(uintptr_t)out;
    const u128 xe = xb + 4 * ((u128)(n_rows - 1) * (u128)ldx + (u128)HW), oe = ob + 4 * ((u128)(n_rows - 1) * (u128)ldo + (u128)HW);
    AUGMENT_REQUIRE(xe <= ((u128)1 << 64) && oe <= ((u128)1 << 64), "%s: rows of ldx=%lld / ldo=%lld do not fit the address space", who, (long long)ldx,
                    (long long)ldo);
    AUGMENT_REQUIRE(xe <= ob || oe <= xb, "%s: out overlaps X (the spans of the two sides, first element to last, must be disjoint)", who);

    const int ipb = HW <= AUGMENT_WAVE_PIXELS ? 4 : 1;
    const int64_t want = (n_rows + ipb - 1) / ipb;
    const int nb = (int)(want < 2048 ? want : 2048);             // 8 blocks on each of the 256 CUs; the loop strides over the rest
    ProfScope ps(s, "augment_rows", 0.0, 8.0 * (double)n_rows * (double)HW);
    AugmentArgs a{X, ldx, out, ldo, theta_in, theta_out, n_rows, (uint64_t)row_base, H, W, HW, ipb, seed, counter, 0.0f, 0.0f, 0.0f, log_lo, log_span};
    if (!theta_in) { a.rotate_deg = p->rotate_deg; a.translate_px = p->translate_px; a.shear_deg = p->shear_deg; }
    DMVAE_LAUNCH(augment_rows_kernel, dim3(nb), dim3(256), 0, s, a);
    return check_launch(who);
}

}  // namespace dmvae
