// Structural similarity (Wang et al. 2004) of image rows on the device: row r compares the `planes` H x W f32 images of X[ix ? ix[r] : r]
// with those of Y[iy ? iy[r] : r] under a separable window g[a][b] = fl(w1[a] * w1[b]), VALID windows only (those wholly inside the image).
// Per window, in this order and with these roundings (f32, every product and sum rounded where it is written):
//   mx = 0;  mx = fmaf(g[a][b], x[a][b], mx)                 a ascending, b ascending inside it; my alike
//   dx = x[a][b] - mx, dy = y[a][b] - my                     the second moments are CENTRED on the window's own means: no E[x^2] - mu^2
//   sxx = fmaf(g, fl(dx * dx), sxx), syy = fmaf(g, fl(dy * dy), syy), sxy = fmaf(g, fl(dx * dy), sxy)        one sequence for all three
//   S = fl(fl(2 fl(mx my) + c1) * fl(2 sxy + c2)) / fl(fl(fl(fl(mx mx) + fl(my my)) + c1) * fl(fl(sxx + syy) + c2))      division correctly rounded
// so S(x, x) == 1.0f in bits (numerator and denominator are the same bits: doubling is exact) and S(x, y) == S(y, x) in bits (every
// product and sum above is taken once and commutes).  ssim[r] = the mean of S over all windows of all planes, sse[r] = sum (x - y)^2 over
// the row.
//   ssim_rows_kernel<WIN>  a WAVE owns a comparison; a workgroup holds `ppw` of them (4 up to 45 x 45, 1 at 64 x 64).  Per plane the wave
//                          stages the two H x W planes in its own LDS slice (coalesced b32 loads; the squared error is summed on the way,
//                          lane l taking elements l, l + 64, ...), then its lanes walk the valid windows in STRIPS of 6 along an output
//                          row: per window row a lane reads the 6 + WIN - 1 values of x and of y ONCE into registers and serves its 6
//                          windows from them -- 2 (WIN + 5) LDS reads per 6 WIN taps instead of 12 WIN -- first for the two means, then for
//                          the three centred moments.  S is summed per lane in f64 in strip order, then across the wave by a fixed
//                          butterfly (an exact sum of the 1.0s of S(x, x)); lane 0 writes the row's two outputs.  Nothing is shared between
//                          comparisons: no atomics on floats, the same bits on every call.
// An ix / iy entry out of range reads nothing: NaN to that comparison's outputs, SSIM_ERR_INDEX OR-ed into *err_flag (an integer atomic).
#include "ssim.h"

namespace dmvae {

constexpr int SSIM_STRIP = 6;                    // windows per lane and pass along an output row (28 - 11 + 1 = 18 = 3 strips)
constexpr int SSIM_LDS_HEAD = 16;                // floats in front of the planes: w1
constexpr int SSIM_LDS_TAIL = 8;                 // floats behind them: what the last row's last strip reads past its plane (< SSIM_STRIP)
constexpr int SSIM_LDS_MAX = 65536;              // the dynamic LDS a launch may ask for without an attribute

// Every product, sum and quotient below is rounded where it is written.  hipcc's default, -ffp-contract=fast, would fuse fl(mx mx) +
// fl(my my) into fmaf(mx, mx, fl(my my)), which is not the bits of fmaf(my, my, fl(mx mx)): the sides would no longer swap.  The
// headers' __fmul_rn / __fadd_rn are plain operators compiled under that default and fuse alike, so the file turns contraction off and
// names its own; fmaf is written out where a fused step is meant.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }      // (correctly rounded: no fast-math flag is passed)

struct SsimArgs {
    const float* X; int64_t ldx; int64_t nx; const int32_t* ix;
    const float* Y; int64_t ldy; int64_t ny; const int32_t* iy;
    int64_t n_pairs;
    int H, W, planes, ppw;
    float c1, c2;
    float w1[SSIM_MAX_WIN];
    float* ssim; float* sse; int32_t* err_flag;
};

template <int WIN>
__global__ __launch_bounds__(256) void ssim_rows_kernel(SsimArgs a) {
    extern __shared__ float ssim_lds[];
    constexpr int S = SSIM_STRIP, NB = WIN + S - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, W = a.W, HW = H * W;
    float* sw = ssim_lds;
    float* px = ssim_lds + SSIM_LDS_HEAD + (size_t)wave * 2 * HW;
    float* py = px + HW;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < WIN; ++t) sw[t] = a.w1[t];
    }
    const int64_t r = (int64_t)blockIdx.x * a.ppw + wave;
    const bool active = r < a.n_pairs;
    int64_t xi = 0, yi = 0;
    if (active) {
        xi = a.ix ? (int64_t)a.ix[r] : r;
        yi = a.iy ? (int64_t)a.iy[r] : r;
    }
    const bool ok = active && xi >= 0 && xi < a.nx && yi >= 0 && yi < a.ny;      // checked before it indexes anything
    const float* xr = a.X + (ok ? xi : 0) * a.ldx;
    const float* yr = a.Y + (ok ? yi : 0) * a.ldy;
    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const int spr = (OW + S - 1) / S, nstrips = OH * spr;
    float sse = 0.f;
    double sum = 0.0;

    for (int p = 0; p < a.planes; ++p) {
        __syncthreads();                                         // the plane before has been read (first round: publishes sw)
        if (ok) {
            const float* xp = xr + (int64_t)p * HW;
            const float* yp = yr + (int64_t)p * HW;
            for (int i = lane; i < HW; i += 64) {
                const float x = xp[i], y = yp[i];
                px[i] = x;
                py[i] = y;
                const float d = sub_rn(x, y);
                sse = fmaf(d, d, sse);
            }
        }
        __syncthreads();
        if (!ok) continue;
        for (int s = lane; s < nstrips; s += 64) {
            const int oy = s / spr, ox0 = (s - oy * spr) * S;
            // (a strip that passes the row's end reads on into the next row, the last row's into the slice behind it or the tail of
            //  the allocation: in bounds, and only windows that are discarded below take those values)
            float mx[S], my[S];
#pragma unroll
            for (int t = 0; t < S; ++t) mx[t] = my[t] = 0.f;
#pragma unroll 1
            for (int wa = 0; wa < WIN; ++wa) {
                const float ga = sw[wa];
                const float* rx = px + (oy + wa) * W + ox0;
                const float* ry = py + (oy + wa) * W + ox0;
                float bx[NB], by[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) { bx[j] = rx[j]; by[j] = ry[j]; }
#pragma unroll
                for (int b = 0; b < WIN; ++b) {
                    const float g = mul_rn(ga, a.w1[b]);
#pragma unroll
                    for (int t = 0; t < S; ++t) {
                        mx[t] = fmaf(g, bx[t + b], mx[t]);
                        my[t] = fmaf(g, by[t + b], my[t]);
                    }
                }
            }
            float sxx[S], syy[S], sxy[S];
#pragma unroll
            for (int t = 0; t < S; ++t) sxx[t] = syy[t] = sxy[t] = 0.f;
#pragma unroll 1
            for (int wa = 0; wa < WIN; ++wa) {
                const float ga = sw[wa];
                const float* rx = px + (oy + wa) * W + ox0;
                const float* ry = py + (oy + wa) * W + ox0;
                float bx[NB], by[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) { bx[j] = rx[j]; by[j] = ry[j]; }
#pragma unroll
                for (int b = 0; b < WIN; ++b) {
                    const float g = mul_rn(ga, a.w1[b]);
#pragma unroll
                    for (int t = 0; t < S; ++t) {
                        const float dx = sub_rn(bx[t + b], mx[t]), dy = sub_rn(by[t + b], my[t]);
                        sxx[t] = fmaf(g, mul_rn(dx, dx), sxx[t]);
                        syy[t] = fmaf(g, mul_rn(dy, dy), syy[t]);
                        sxy[t] = fmaf(g, mul_rn(dx, dy), sxy[t]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < S; ++t) {
                if (ox0 + t < OW) {
                    const float a1 = add_rn(mul_rn(2.f, mul_rn(mx[t], my[t])), a.c1);
                    const float a2 = add_rn(mul_rn(2.f, sxy[t]), a.c2);
                    const float b1 = add_rn(add_rn(mul_rn(mx[t], mx[t]), mul_rn(my[t], my[t])), a.c1);
                    const float b2 = add_rn(add_rn(sxx[t], syy[t]), a.c2);
                    sum += (double)div_rn(mul_rn(a1, a2), mul_rn(b1, b2));
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        sse += __shfl_xor(sse, o, 64);
    }
    if (lane == 0) {
        if (ok) {
            a.ssim[r] = (float)(sum / (double)((int64_t)a.planes * OH * OW));
            if (a.sse) a.sse[r] = sse;
        } else {
            a.ssim[r] = __int_as_float(0x7fc00000);
            if (a.sse) a.sse[r] = __int_as_float(0x7fc00000);
            if (a.err_flag) atomicOr(a.err_flag, SSIM_ERR_INDEX);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define SSIM_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return DMVAE_EINVAL; } } while (0)

int ssim_rows_launch(hipStream_t s, const float* X, int64_t ldx, int64_t nx, const int32_t* ix, const float* Y, int64_t ldy, int64_t ny, const int32_t* iy,
                     int64_t n_pairs, int H, int W, int planes, const float* w1, int win, float c1, float c2, float* ssim, float* sse, int32_t* err_flag) {
    const char* who = "dmvae_ssim_rows";
    SSIM_REQUIRE(X && Y && ssim && w1, "%s: null X / Y / ssim / w1", who);
    SSIM_REQUIRE(n_pairs >= 1 && nx >= 1 && ny >= 1, "%s: n_pairs=%lld, nx=%lld, ny=%lld (all >= 1)", who, (long long)n_pairs, (long long)nx, (long long)ny);
    SSIM_REQUIRE(H >= 1 && W >= 1 && planes >= 1, "%s: H=%d, W=%d, planes=%d (all >= 1)", who, H, W, planes);
    SSIM_REQUIRE(win >= 3 && win <= SSIM_MAX_WIN && (win & 1) && win <= H && win <= W, "%s: win=%d (odd, 3 .. %d, at most min(H, W) = %d)", who, win,
                 SSIM_MAX_WIN, H < W ? H : W);
    if ((int64_t)H * W > SSIM_MAX_HW) {
        set_error("%s: H*W = %lld exceeds %d (the two planes of a pair are held in 32 KiB of LDS)", who, (long long)H * W, SSIM_MAX_HW);
        return DMVAE_EUNSUPPORTED;
    }
    const int HW = H * W;
    const int64_t row = (int64_t)planes * HW;
    SSIM_REQUIRE(ldx >= row && ldy >= row, "%s: ldx=%lld, ldy=%lld (both >= planes*H*W = %lld)", who, (long long)ldx, (long long)ldy, (long long)row);
    int ppw = (SSIM_LDS_MAX - (SSIM_LDS_HEAD + SSIM_LDS_TAIL) * 4) / (8 * HW);
    ppw = ppw > 4 ? 4 : ppw;                                     // >= 1: 8 * 4096 + 96 <= 65536
    const int64_t groups = (n_pairs + ppw - 1) / ppw;
    SSIM_REQUIRE(groups <= 0x7fffffffLL, "%s: n_pairs=%lld needs more than 2^31 - 1 workgroups", who, (long long)n_pairs);
    SsimArgs a{X, ldx, nx, ix, Y, ldy, ny, iy, n_pairs, H, W, planes, ppw, c1, c2, {}, ssim, sse, err_flag};
    for (int t = 0; t < win; ++t) a.w1[t] = w1[t];               // read here, at call time: the weights travel in the argument struct
    const size_t lds = (size_t)(SSIM_LDS_HEAD + SSIM_LDS_TAIL) * 4 + (size_t)ppw * 8 * HW;
    const double windows = (double)n_pairs * planes * (H - win + 1) * (W - win + 1);
    ProfScope ps(s, "ssim_rows", windows * win * win * 20.0, (double)n_pairs * (8.0 * row + 8.0));
    const dim3 grid((unsigned)groups), block(64 * ppw);
    switch (win) {
        case 3: DMVAE_LAUNCH(ssim_rows_kernel<3>, grid, block, lds, s, a); break;
        case 5: DMVAE_LAUNCH(ssim_rows_kernel<5>, grid, block, lds, s, a); break;
        case 7: DMVAE_LAUNCH(ssim_rows_kernel<7>, grid, block, lds, s, a); break;
        case 9: DMVAE_LAUNCH(ssim_rows_kernel<9>, grid, block, lds, s, a); break;
        default: DMVAE_LAUNCH(ssim_rows_kernel<11>, grid, block, lds, s, a); break;
    }
    return check_launch(who);
}

}  // namespace dmvae
