// Sparse-convolution forward of the reference's PreconditionerSparseUNet (uibk/deep_preconditioning/model.py:62-179) for
// gfx950 (MI355X, wave64): the U-Net variant of the network whose output IS the preconditioner's L factor.  The torch
// restatement of the same modules is deeppreconditioning_amd/extras_unet.py; nothing of spconv is used or translated.
//
// Five site sets (levels): S0 = the input sites (one per stored entry (batch, row, col) of tril(A), padding diagonal
// included), S1 .. S4 = the outputs of the four stride-2, padding-1, 3 x 3 convolutions down1, down2, down3, bottleneck.
// Seventeen layers:
//   enc1 / dec0 (S0), enc2 / dec1 (S1), enc3 / dec2 (S2), enc4 / dec3 (S3): 3 x 3 submanifold convolutions, + LeakyReLU;
//   down1 .. bottleneck: S_l -> S_l+1, + LeakyReLU;
//   up3 .. up0: inverse convolutions, S_l+1 -> S_l through the rulebook of the stride-2 convolution S_l -> S_l+1 read
//     backwards, + LeakyReLU, + the skip (sparse_add with the encoder output on S_l: the same site set, so a plain sum);
//   out_conv: pointwise c[1] -> c[5] on S0, then model.py:169-173 on every channel (strict upper part zeroed, softplus on
//     the diagonal).
//
//   plan (once per sparsity pattern: dpcg_unet_plan_create / _rebuild).  Every level is CSR over the image rows (rowptr
//     over batch * height rows, sorted columns).  S_l+1 is built row by row: one thread per OUTPUT row merges the 9 input
//     lists that can feed it -- input row 2 * oy + ky - 1, input column x through tap kx reaching output column
//     (x - kx + 1) / 2 when that is even -- in two passes (count, scan, fill).  The fill pass writes the rulebook in both
//     forms: nbr[o][t] (output-stationary, for the down layer) and its transpose dst[i][t] (input-stationary, for the
//     inverse convolution).  Each (input site, tap) pair feeds at most one output site, so the transpose is a scatter
//     without conflicts.  The submanifold rulebook of a level (shared by its encoder and decoder layer, as spconv's
//     indice_key shares it) is one thread per row walking the three neighbouring rows.  No sort, no hash table, no
//     atomics: every array is a deterministic function of the pattern.
//   forward (dpcg_unet_forward).  Every 3 x 3 layer is out[o, :] = act(bias + sum_t in[nbr[o][t], :] W_t) (+ skip[o, :]):
//     a gathered GEMM with M = sites, K = 9 * C_in, N = C_out on v_mfma_f32_16x16x4_f32 when C_in, C_out are 16 / 32 / 64,
//     one thread per (site, channel) otherwise.  Each output element has one writer: the result is bitwise reproducible.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "dpcg_host.h"
#include "dpcg_prims.h"
#include "dpcg_sconv.h"

namespace dpcg {
namespace {

constexpr int kUnetLevels = 5;       // S0 .. S4
constexpr int kUnetLayers = 17;      // enc1 down1 enc2 down2 enc3 down3 enc4 bottleneck up3 dec3 up2 dec2 up1 dec1 up0 dec0 out_conv
constexpr int kTaps = 9;             // 3 x 3 windows
constexpr int kUnetBlock = 512;      // MFMA kernel: 8 waves, so that one workgroup per CU (64 x 64 weights: 144 KiB of LDS) still has two per SIMD

struct UnetLevel {
    int64_t h = 0, w = 0, sites = 0;
    int32_t *rowptr = nullptr;       // [batch * h + 1]
    int32_t *col = nullptr;          // [sites]
    int32_t *subm = nullptr;         // [sites * 9] submanifold rulebook: site of this level at (y + ky - 1, x + kx - 1), -1 = none (levels 0-3)
    int32_t *down = nullptr;         // [sites * 9] stride-2 rulebook INTO this level: input site of level - 1 per tap, -1 = none (levels 1-4)
    int32_t *up = nullptr;           // [sites * 9] its transpose FROM this level: site of level + 1 this site feeds per tap, -1 = none (levels 0-3)
};

}  // namespace
}  // namespace dpcg

struct dpcg_unet_plan {
    int batch = 0;
    bool ready = false;
    dpcg::UnetLevel lv[dpcg::kUnetLevels];
    int32_t *site_row = nullptr;      // [S0] image row of every input site
    int32_t *site_batch = nullptr;    // [S0]
    int32_t *lower_rowptr = nullptr;  // [batch * height + 1] the lower-triangular CSR (col <= row) of S0
    int32_t *lower_col = nullptr;
    int32_t *lower_pos = nullptr;     // [S0] position in the lower CSR, -1 for col > row
    int64_t nnz_lower = 0;
    // hidden features: enc1 .. enc4 (kept for the skips) and two scratch buffers, grown on demand
    float *buf[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t buf_cap[6] = {0, 0, 0, 0, 0, 0};
    // every pattern-sized array lives in these slabs (dpcg_sconv.h plan_alloc): a rebuild allocates nothing it already has
    std::vector<std::pair<void *, size_t>> slabs;
    size_t slab_cursor = 0;
};

namespace dpcg {
namespace {

// ---- plan kernels ----------------------------------------------------------------------------------------------
// Submanifold rulebook of one level: one thread per row.  The three neighbouring rows are walked with cursors that only
// move forward (a row's sites are sorted, so the first column >= x - 1 of a neighbouring row never moves back).
__global__ __launch_bounds__(kBlock) void k_subm_rows(int batch, int64_t H, const int32_t *__restrict__ rp,
                                                      const int32_t *__restrict__ col, int32_t *__restrict__ nbr) {
    const int64_t rows = (int64_t)batch * H;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
        const int64_t b = r / H, y = r - b * H;
        int beg[3], end[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int64_t yy = y + ky - 1;
            beg[ky] = end[ky] = 0;
            if (yy >= 0 && yy < H) {
                beg[ky] = rp[b * H + yy];
                end[ky] = rp[b * H + yy + 1];
            }
        }
        for (int k = rp[r]; k < rp[r + 1]; ++k) {
            const int x = col[k];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                int p = beg[ky];
                while (p < end[ky] && col[p] < x - 1) ++p;
                beg[ky] = p;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int target = x + kx - 1;
                    while (p < end[ky] && col[p] < target) ++p;
                    nbr[(int64_t)k * kTaps + ky * 3 + kx] = (p < end[ky] && col[p] == target) ? p : -1;
                }
            }
        }
    }
}

struct DownGeom {
    int batch;
    int64_t h_in, w_in, h_out, w_out;
};

// Stride-2, padding-1, 3 x 3: one thread per OUTPUT row oy merges the 9 lists t = (ky, kx): input row 2 oy + ky - 1, and of
// its sites those whose column x makes x - kx + 1 even and >= 0; such a site reaches output column (x - kx + 1) / 2.  Each
// list is sorted by that column and holds it at most once.  FILL = false: len[r] = distinct output columns.  FILL = true:
// columns, the rulebook nbr[o][t] and its transpose dst[i][t] (which the caller set to -1 beforehand).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_down_rows(DownGeom g, const int32_t *__restrict__ rp_in,
                                                      const int32_t *__restrict__ col_in, int32_t *__restrict__ len,
                                                      const int32_t *__restrict__ rp_out, int32_t *__restrict__ col_out,
                                                      int32_t *__restrict__ nbr, int32_t *__restrict__ dst) {
    const int64_t rows_out = (int64_t)g.batch * g.h_out;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r <= rows_out; r += stride) {
        if (r == rows_out) {
            if (!FILL) len[r] = 0;
            continue;
        }
        const int64_t b = r / g.h_out, oy = r - b * g.h_out;
        int cur[kTaps], end[kTaps];
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            const int ky = t / 3, kx = t - 3 * (t / 3);
            const int64_t y = 2 * oy + ky - 1;
            cur[t] = end[t] = 0;
            if (y >= 0 && y < g.h_in) {
                cur[t] = rp_in[b * g.h_in + y];
                end[t] = rp_in[b * g.h_in + y + 1];
            }
            while (cur[t] < end[t] && ((col_in[cur[t]] + 1 - kx) < 0 || ((col_in[cur[t]] + 1 - kx) & 1))) ++cur[t];
        }
        int count = 0;
        int64_t at = FILL ? rp_out[r] : 0;
        for (;;) {
            int best = 0x7fffffff;
#pragma unroll
            for (int t = 0; t < kTaps; ++t)
                if (cur[t] < end[t]) {
                    const int v = (col_in[cur[t]] + 1 - t % 3) >> 1;
                    best = v < best ? v : best;
                }
            if (best == 0x7fffffff || best >= g.w_out) break;      // exhausted, or clipped on the right (sorted)
            if (FILL) col_out[at] = best;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const int kx = t % 3;
                int src = -1;
                if (cur[t] < end[t] && ((col_in[cur[t]] + 1 - kx) >> 1) == best) {
                    src = cur[t]++;
                    while (cur[t] < end[t] && ((col_in[cur[t]] + 1 - kx) & 1)) ++cur[t];
                }
                if (FILL) {
                    nbr[at * kTaps + t] = src;
                    if (src >= 0) dst[(int64_t)src * kTaps + t] = (int32_t)at;
                }
            }
            ++at;
            ++count;
        }
        if (!FILL) len[r] = count;
    }
}

// (sites, 3) indices of one level, one thread per row
__global__ __launch_bounds__(kBlock) void k_level_indices(int64_t rows, int64_t H, const int32_t *__restrict__ rp,
                                                          const int32_t *__restrict__ col, int32_t *__restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
        const int b = (int)(r / H), y = (int)(r % H);
        for (int k = rp[r]; k < rp[r + 1]; ++k) {
            idx[3 * (int64_t)k] = b;
            idx[3 * (int64_t)k + 1] = y;
            idx[3 * (int64_t)k + 2] = col[k];
        }
    }
}

// ---- forward kernels -------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float leaky(float v, float slope) { return v >= 0.f ? v : slope * v; }

// 3 x 3 sparse convolution (any of the three kinds: the rulebook says which) as a gathered GEMM on v_mfma_f32_16x16x4_f32.
// One wave = 16 output sites x COUT channels.  Lane l = (m = l & 15, q = l >> 4).  K = 9 taps x CIN channels is walked tap
// by tap; inside a tap, instruction (u, e) puts channel 16 u + 4 q + e in K-quarter q, so a lane's A operands for one tap
// are CIN / 16 16-byte loads of ONE neighbour's feature row (channels 16 u + 4 q .. + 3), and no K slot is padding.
// B operand = W_t[ci][co] from LDS, the whole 9 x CIN x COUT block staged once per workgroup in the order
// [t][u][e][q][m][nb] (co = 16 nb + m): a lane reads its NB = COUT / 16 values of one instruction as one 4 * NB-byte word,
// and the lane groups of ds_read_b32 / _b64 / _b128 meet distinct banks.  The next tap's feature loads (and the rulebook
// entry of the tap after it) are in flight while this tap's matrix instructions issue.  Epilogue: bias, LeakyReLU, then
// (SKIP) the encoder output of the same site -- the order of model.py:152-165 (act, then sparse_add).
template <int CIN, int COUT, bool SKIP>
__global__ __launch_bounds__(kUnetBlock) void k_unet_conv3x3_mfma(int64_t n_out, const int32_t *__restrict__ nbr,
                                                                 const float *__restrict__ in, const float *__restrict__ w,
                                                                 const float *__restrict__ bias, float slope,
                                                                 const float *__restrict__ skip, float *__restrict__ out) {
    constexpr int NB = COUT / 16, U = CIN / 16;
    __shared__ __attribute__((aligned(16))) float wl[kTaps * CIN * COUT];
    // w is KRSC: w[co][t][ci]
    for (int e = threadIdx.x; e < COUT * kTaps * CIN; e += kUnetBlock) {
        const int co = e / (kTaps * CIN), rem = e - co * kTaps * CIN, t = rem / CIN, ci = rem - t * CIN;
        const int u = ci >> 4, q = (ci >> 2) & 3, ee = ci & 3;
        wl[((((t * U + u) * 4 + ee) * 4 + q) * 16 + (co & 15)) * NB + (co >> 4)] = w[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    float bias_r[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bias_r[nb] = bias ? bias[nb * 16 + m] : 0.f;
    const float *wq = wl + (q * 16 + m) * NB;
    constexpr int kWaves = kUnetBlock / 64;
    const int64_t n_tiles = (n_out + 15) >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
        const int64_t o = tile * 16 + m;
        const bool live = o < n_out;
        const int32_t *nb_o = nbr + (live ? o : 0) * kTaps;
        // NB == 1: two accumulator chains (even / odd e) keep the matrix pipe issuing every 32 cycles (40-cycle dependent latency)
        constexpr int CH = NB == 1 ? 2 : NB;
        f32x4 acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = zero;
        f32x4 cur[U], nxt[U];
        int s_next = live ? nb_o[1] : -1;
        {
            const int s0 = live ? nb_o[0] : -1;
            const f32x4 *p = reinterpret_cast<const f32x4 *>(in + (int64_t)(s0 < 0 ? 0 : s0) * CIN) + q;
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = s0 < 0 ? zero : p[4 * u];
        }
#pragma unroll 1
        for (int t = 0; t < kTaps; ++t) {
            if (t + 1 < kTaps) {
                const int s1 = s_next;
                const f32x4 *p = reinterpret_cast<const f32x4 *>(in + (int64_t)(s1 < 0 ? 0 : s1) * CIN) + q;
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = s1 < 0 ? zero : p[4 * u];
                s_next = (live && t + 2 < kTaps) ? nb_o[t + 2] : -1;
            }
            const float *wt = wq + t * U * 4 * 64 * NB;
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = cur[u][e];
                    const float *wp = wt + (u * 4 + e) * 64 * NB;
                    float bv[NB];
                    if constexpr (NB == 4) {
                        const f32x4 v = *reinterpret_cast<const f32x4 *>(wp);
                        bv[0] = v[0]; bv[1] = v[1]; bv[2] = v[2]; bv[3] = v[3];
                    } else if constexpr (NB == 2) {
                        const float2 v = *reinterpret_cast<const float2 *>(wp);
                        bv[0] = v.x; bv[1] = v.y;
                    } else {
                        bv[0] = wp[0];
                    }
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const int c = NB == 1 ? (e & 1) : nb;
                        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[nb], acc[c], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t row = tile * 16 + q * 4 + i;
                if (row < n_out) {
                    float v = leaky((NB == 1 ? acc[0][i] + acc[1][i] : acc[nb][i]) + bias_r[nb], slope);
                    if (SKIP) v += skip[row * COUT + nb * 16 + m];
                    out[row * COUT + nb * 16 + m] = v;
                }
            }
        }
    }
}

// Any channel counts (the first layer has ONE input channel; small nets): one thread per (site, output channel), plain
// fp32 FMAs in the order tap-major, channel-minor; the same epilogue.
template <bool SKIP>
__global__ __launch_bounds__(kBlock) void k_unet_conv_generic(int64_t n_out, const int32_t *__restrict__ nbr, int cin, int cout,
                                                              const float *__restrict__ in, const float *__restrict__ w,
                                                              const float *__restrict__ bias, float slope,
                                                              const float *__restrict__ skip, float *__restrict__ out) {
    const int64_t total = n_out * cout, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
        const int64_t o = e / cout;
        const int co = (int)(e - o * cout);
        float s = bias ? bias[co] : 0.f;
        for (int t = 0; t < kTaps; ++t) {
            const int64_t src = nbr[o * kTaps + t];
            if (src < 0) continue;
            const float *__restrict__ f = in + src * cin;
            const float *__restrict__ wk = w + ((int64_t)co * kTaps + t) * cin;
            for (int ci = 0; ci < cin; ++ci) s = fmaf(f[ci], wk[ci], s);
        }
        s = leaky(s, slope);
        if (SKIP) s += skip[e];
        out[e] = s;
    }
}

// out_conv (pointwise, C_in -> C_out) + model.py:169-173 on every channel: strict upper part zeroed, softplus on the diagonal
// (torch's: x > 20 ? x : log1p(exp(x))).  Writes the (sites, C_out) features and channel 0, for col <= row, as the fp64
// value of L in the lower-triangular CSR.  One thread per (site, output channel).
__global__ __launch_bounds__(kBlock) void k_unet_out(int64_t sites, int cin, int cout, const float *__restrict__ in,
                                                     const float *__restrict__ w, const float *__restrict__ bias,
                                                     const int32_t *__restrict__ site_row, const int32_t *__restrict__ col,
                                                     const int32_t *__restrict__ lpos, float *__restrict__ feat_out,
                                                     double *__restrict__ lower_val) {
    const int64_t total = sites * cout, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / cout;
        const int co = (int)(e - i * cout);
        const float *__restrict__ f = in + i * cin;
        const float *__restrict__ wk = w + (int64_t)co * cin;
        float s = bias ? bias[co] : 0.f;
        for (int ci = 0; ci < cin; ++ci) s = fmaf(f[ci], wk[ci], s);
        const int y = site_row[i], x = col[i];
        if (y < x) s = 0.f;
        else if (y == x) s = s > 20.f ? s : log1pf(expf(s));
        if (feat_out) feat_out[e] = s;
        if (lower_val && co == 0) {
            const int at = lpos[i];
            if (at >= 0) lower_val[at] = (double)s;
        }
    }
}

// The same for C_in = 16 / 32 / 64: one thread per site reads its feature row once (16-byte loads) and makes every output
// channel from it; the weights are the same for all lanes (scalar loads).  Same order of operations as k_unet_out.
template <int CIN>
__global__ __launch_bounds__(kBlock) void k_unet_out_rows(int64_t sites, int cout, const float *__restrict__ in,
                                                          const float *__restrict__ w, const float *__restrict__ bias,
                                                          const int32_t *__restrict__ site_row, const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ lpos, float *__restrict__ feat_out,
                                                          double *__restrict__ lower_val) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < sites; i += stride) {
        float f[CIN];
        const f32x4 *__restrict__ p = reinterpret_cast<const f32x4 *>(in + i * CIN);
#pragma unroll
        for (int u = 0; u < CIN / 4; ++u) {
            const f32x4 v = p[u];
            f[4 * u] = v[0]; f[4 * u + 1] = v[1]; f[4 * u + 2] = v[2]; f[4 * u + 3] = v[3];
        }
        const int y = site_row[i], x = col[i];
        for (int co = 0; co < cout; ++co) {
            const float *__restrict__ wk = w + (int64_t)co * CIN;
            float s = bias ? bias[co] : 0.f;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) s = fmaf(f[ci], wk[ci], s);
            if (y < x) s = 0.f;
            else if (y == x) s = s > 20.f ? s : log1pf(expf(s));
            if (feat_out) feat_out[i * cout + co] = s;
            if (lower_val && co == 0) {
                const int at = lpos[i];
                if (at >= 0) lower_val[at] = (double)s;
            }
        }
    }
}

template <int CIN, int COUT>
void launch_unet_mfma(int64_t n_out, const int32_t *nbr, const float *in, const float *w, const float *bias, float slope,
                      const float *skip, float *out, hipStream_t s) {
    constexpr int lds = kTaps * CIN * COUT * 4;
    constexpr int per_cu = (160 * 1024) / lds < 1 ? 1 : ((160 * 1024) / lds > 4 ? 4 : (160 * 1024) / lds);
    const int64_t tiles = (n_out + 15) / 16;
    int64_t g = (tiles + kUnetBlock / 64 - 1) / (kUnetBlock / 64);
    if (g > 256 * per_cu) g = 256 * per_cu;
    if (g < 1) g = 1;
    if (skip)
        hipLaunchKernelGGL((k_unet_conv3x3_mfma<CIN, COUT, true>), dim3((int)g), dim3(kUnetBlock), 0, s, n_out, nbr, in, w, bias,
                           slope, skip, out);
    else
        hipLaunchKernelGGL((k_unet_conv3x3_mfma<CIN, COUT, false>), dim3((int)g), dim3(kUnetBlock), 0, s, n_out, nbr, in, w, bias,
                           slope, skip, out);
}

// one 3 x 3 layer: the MFMA kernel when one exists for (cin, cout), the generic one otherwise
void unet_conv(int cin, int cout, int64_t n_out, const int32_t *nbr, const float *in, const float *w, const float *bias,
               float slope, const float *skip, float *out, hipStream_t s) {
#define DPCG_UNET_CASE(CI, CO)                                                  \
    if (cin == CI && cout == CO) {                                              \
        launch_unet_mfma<CI, CO>(n_out, nbr, in, w, bias, slope, skip, out, s); \
        return;                                                                 \
    }
    DPCG_UNET_CASE(16, 16) DPCG_UNET_CASE(16, 32) DPCG_UNET_CASE(16, 64)
    DPCG_UNET_CASE(32, 16) DPCG_UNET_CASE(32, 32) DPCG_UNET_CASE(32, 64)
    DPCG_UNET_CASE(64, 16) DPCG_UNET_CASE(64, 32) DPCG_UNET_CASE(64, 64)
#undef DPCG_UNET_CASE
    const int g = grid_blocks(n_out * cout, kConvGrid);
    if (skip)
        hipLaunchKernelGGL((k_unet_conv_generic<true>), dim3(g), dim3(kBlock), 0, s, n_out, nbr, cin, cout, in, w, bias, slope,
                           skip, out);
    else
        hipLaunchKernelGGL((k_unet_conv_generic<false>), dim3(g), dim3(kBlock), 0, s, n_out, nbr, cin, cout, in, w, bias, slope,
                           skip, out);
}

}  // namespace
}  // namespace dpcg

using namespace dpcg;

extern "C" int dpcg_unet_plan_destroy(dpcg_unet_plan_t p) {
    if (!p) return DPCG_OK;
    for (auto &sl : p->slabs)
        if (sl.first) (void)device_free(sl.first);
    for (auto &b : p->buf) dev_free(b);
    delete p;
    return DPCG_OK;
}

// (Re)builds `p` for a pattern, drawing its arrays from the plan's slabs.  On failure the plan is left EMPTY (ready = false)
// but alive: its memory can serve the next rebuild.
static int build_unet_plan(dpcg_unet_plan *p, int batch, int64_t height, int64_t width, int64_t nnz, const int32_t *indices,
                           dpcg_stream_t stream) {
    p->ready = false;
    if (batch <= 0 || height <= 0 || width <= 0 || nnz <= 0 || !indices)
        return invalid("dpcg_unet_plan_create: bad arguments");
    if ((int64_t)batch * height >= 2147483000LL || nnz >= 2147483000LL || width >= 2147483000LL)
        return invalid("dpcg_unet_plan_create: batch * height, width or nnz exceeds int32");
    hipStream_t s = (hipStream_t)stream;
    p->slab_cursor = 0;
    p->batch = batch;
    p->nnz_lower = 0;
    for (auto &L : p->lv) L = UnetLevel();
    int st = DPCG_OK;
    int *d_bad = nullptr;
    int32_t *len = nullptr;
    void *scan_ws = nullptr;
    const int64_t max_rows = (int64_t)batch * height + 1;       // the levels below S0 have fewer rows
    const size_t scan_bytes = scan_workspace_bytes(max_rows) + 256;
#define PLAN_TRY(expr)            \
    do {                          \
        st = (expr);              \
        if (st < 0) return st;    \
    } while (0)
#define PLAN_HIP(call)                                                \
    do {                                                              \
        hipError_t _e = (call);                                       \
        if (_e != hipSuccess) return hip_fail(_e, #call, __FILE__, __LINE__); \
    } while (0)
    UnetLevel &L0 = p->lv[0];
    L0.h = height;
    L0.w = width;
    L0.sites = nnz;
    const int64_t rows0 = (int64_t)batch * height;
    PLAN_TRY(plan_alloc(p, &L0.rowptr, rows0 + 1));
    PLAN_TRY(plan_alloc(p, &L0.col, nnz));
    PLAN_TRY(plan_alloc(p, &d_bad, 1));
    PLAN_TRY(plan_alloc(p, reinterpret_cast<char **>(&scan_ws), (int64_t)scan_bytes));
    PLAN_TRY(plan_alloc(p, &len, max_rows));
    PLAN_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_sites_to_csr, dim3(grid_blocks(nnz, kConvGrid)), dim3(kBlock), 0, s, nnz, indices, batch, height, width, L0.rowptr,
                       L0.col, d_bad);
    int bad = 0;
    PLAN_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PLAN_HIP(hipStreamSynchronize(s));
    if (bad) {
        set_error(bad == 1 ? "dpcg_unet_plan_create: a site lies outside the batch / image"
                           : "dpcg_unet_plan_create: sites must be sorted by (batch, row, col) without duplicates");
        return DPCG_ERR_INVALID;
    }
    for (int l = 0; l + 1 < kUnetLevels; ++l) {
        UnetLevel &A = p->lv[l], &B = p->lv[l + 1];
        B.h = (A.h - 1) / 2 + 1;       // (h + 2 * 1 - 3) / 2 + 1
        B.w = (A.w - 1) / 2 + 1;
        const int64_t rows_a = (int64_t)batch * A.h, rows_b = (int64_t)batch * B.h;
        // submanifold rulebook of level l (enc and dec share it)
        PLAN_TRY(plan_alloc(p, &A.subm, A.sites * kTaps));
        hipLaunchKernelGGL(k_subm_rows, dim3(grid_blocks(rows_a, kConvGrid)), dim3(kBlock), 0, s, batch, A.h, (const int32_t *)A.rowptr,
                           (const int32_t *)A.col, A.subm);
        // S_l+1 and the stride-2 rulebook in both forms
        const DownGeom g{batch, A.h, A.w, B.h, B.w};
        PLAN_TRY(plan_alloc(p, &B.rowptr, rows_b + 1));
        hipLaunchKernelGGL(k_down_rows<false>, dim3(grid_blocks(rows_b + 1, kConvGrid)), dim3(kBlock), 0, s, g, (const int32_t *)A.rowptr,
                           (const int32_t *)A.col, len, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                           (int32_t *)nullptr);
        PLAN_TRY(exclusive_scan_i32_ws(len, B.rowptr, rows_b + 1, scan_ws, scan_bytes, s));
        int32_t total = 0;
        PLAN_HIP(hipMemcpyAsync(&total, B.rowptr + rows_b, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PLAN_HIP(hipStreamSynchronize(s));
        if (total <= 0) {
            set_error("dpcg_unet_plan_create: a level has no active site (or more than 2^31)");
            return DPCG_ERR_INVALID;
        }
        B.sites = total;
        PLAN_TRY(plan_alloc(p, &B.col, B.sites));
        PLAN_TRY(plan_alloc(p, &B.down, B.sites * kTaps));
        PLAN_TRY(plan_alloc(p, &A.up, A.sites * kTaps));
        PLAN_HIP(hipMemsetAsync(A.up, 0xff, (size_t)A.sites * kTaps * sizeof(int32_t), s));
        hipLaunchKernelGGL(k_down_rows<true>, dim3(grid_blocks(rows_b + 1, kConvGrid)), dim3(kBlock), 0, s, g, (const int32_t *)A.rowptr,
                           (const int32_t *)A.col, (int32_t *)nullptr, (const int32_t *)B.rowptr, B.col, B.down, A.up);
    }
    // rows of the input sites and the lower-triangular CSR the factor is written into
    PLAN_TRY(plan_alloc(p, &p->site_row, nnz));
    PLAN_TRY(plan_alloc(p, &p->site_batch, nnz));
    PLAN_TRY(plan_alloc(p, &p->lower_rowptr, rows0 + 1));
    PLAN_TRY(plan_alloc(p, &p->lower_pos, nnz));
    hipLaunchKernelGGL(k_lower_count, dim3(grid_blocks(rows0 + 1, kConvGrid)), dim3(kBlock), 0, s, rows0, height, (const int32_t *)L0.rowptr,
                       (const int32_t *)L0.col, len, p->site_row, p->site_batch);
    PLAN_TRY(exclusive_scan_i32_ws(len, p->lower_rowptr, rows0 + 1, scan_ws, scan_bytes, s));
    int32_t total = 0;
    PLAN_HIP(hipMemcpyAsync(&total, p->lower_rowptr + rows0, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PLAN_HIP(hipStreamSynchronize(s));
    p->nnz_lower = total;
    PLAN_TRY(plan_alloc(p, &p->lower_col, p->nnz_lower));
    hipLaunchKernelGGL(k_lower_fill, dim3(grid_blocks(rows0, kConvGrid)), dim3(kBlock), 0, s, rows0, height, (const int32_t *)L0.rowptr,
                       (const int32_t *)L0.col, (const int32_t *)p->lower_rowptr, p->lower_col, p->lower_pos);
    PLAN_HIP(hipStreamSynchronize(s));
    PLAN_HIP(hipGetLastError());
#undef PLAN_TRY
#undef PLAN_HIP
    p->ready = true;
    return DPCG_OK;
}

extern "C" int dpcg_unet_plan_create(dpcg_unet_plan_t *out, int batch, int64_t height, int64_t width, int64_t nnz,
                                     const int32_t *indices, dpcg_stream_t stream) {
    if (!out) return invalid("dpcg_unet_plan_create: NULL out");
    *out = nullptr;
    dpcg_unet_plan *p = new dpcg_unet_plan();
    const int st = build_unet_plan(p, batch, height, width, nnz, indices, stream);
    if (st < 0) {
        dpcg_unet_plan_destroy(p);
        return st;
    }
    *out = p;
    return DPCG_OK;
}

extern "C" int dpcg_unet_plan_rebuild(dpcg_unet_plan_t plan, int batch, int64_t height, int64_t width, int64_t nnz,
                                      const int32_t *indices, dpcg_stream_t stream) {
    if (!plan) return invalid("dpcg_unet_plan_rebuild: NULL plan");
    return build_unet_plan(plan, batch, height, width, nnz, indices, stream);
}

extern "C" int dpcg_unet_plan_info(dpcg_unet_plan_t p, int level, int64_t *sites, int64_t *height, int64_t *width,
                                   int64_t *nnz_lower) {
    if (!p || !p->ready || level < 0 || level >= kUnetLevels)
        return invalid("dpcg_unet_plan_info: bad plan or level (or a plan whose rebuild failed)");
    const UnetLevel &L = p->lv[level];
    if (sites) *sites = L.sites;
    if (height) *height = L.h;
    if (width) *width = L.w;
    if (nnz_lower) *nnz_lower = p->nnz_lower;
    return DPCG_OK;
}

extern "C" int dpcg_unet_plan_level_indices(dpcg_unet_plan_t p, int level, int32_t *indices_out, dpcg_stream_t stream) {
    if (!p || !p->ready || level < 0 || level >= kUnetLevels || !indices_out)
        return invalid("dpcg_unet_plan_level_indices: bad plan, level or output");
    const UnetLevel &L = p->lv[level];
    const int64_t rows = (int64_t)p->batch * L.h;
    hipLaunchKernelGGL(k_level_indices, dim3(grid_blocks(rows, kConvGrid)), dim3(kBlock), 0, (hipStream_t)stream, rows, L.h,
                       (const int32_t *)L.rowptr, (const int32_t *)L.col, indices_out);
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

extern "C" int dpcg_unet_plan_output(dpcg_unet_plan_t p, int32_t *indices_out, int32_t *lower_rowptr, int32_t *lower_col,
                                     dpcg_stream_t stream) {
    if (!p || !p->ready) return invalid("dpcg_unet_plan_output: NULL or empty plan");
    hipStream_t s = (hipStream_t)stream;
    const UnetLevel &L = p->lv[0];
    if (indices_out)
        hipLaunchKernelGGL(k_out_indices, dim3(grid_blocks(L.sites, kConvGrid)), dim3(kBlock), 0, s, L.sites, (const int32_t *)p->site_batch,
                           (const int32_t *)p->site_row, (const int32_t *)L.col, indices_out);
    if (lower_rowptr)
        DPCG_HIP(hipMemcpyAsync(lower_rowptr, p->lower_rowptr, (size_t)((int64_t)p->batch * L.h + 1) * sizeof(int32_t),
                                hipMemcpyDeviceToDevice, s));
    if (lower_col)
        DPCG_HIP(hipMemcpyAsync(lower_col, p->lower_col, (size_t)p->nnz_lower * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

extern "C" int dpcg_unet_forward(dpcg_unet_plan_t p, const int32_t *channels, const int32_t *layer_dims,
                                 const float *const *weights, const float *const *biases, const float *slopes,
                                 const float *features_in, int in_channels, float *features_out, double *lower_val,
                                 dpcg_stream_t stream) {
    if (!p || !channels || !layer_dims || !weights || !biases || !slopes || !features_in)
        return invalid("dpcg_unet_forward: NULL argument");
    if (!p->ready) return invalid("dpcg_unet_forward: empty plan (its last rebuild failed)");
    if (!features_out && !lower_val) return invalid("dpcg_unet_forward: no output");
    const int *c = channels;
    for (int l = 0; l < 6; ++l)
        if (c[l] < 1 || c[l] > 1024) return invalid("dpcg_unet_forward: bad channel count");
    // (C_in, C_out) of every layer as the structure implies it
    const int expect[kUnetLayers][2] = {{c[0], c[1]}, {c[1], c[2]}, {c[2], c[2]}, {c[2], c[3]}, {c[3], c[3]}, {c[3], c[4]},
                                        {c[4], c[4]}, {c[4], c[5]}, {c[5], c[4]}, {c[4], c[4]}, {c[4], c[3]}, {c[3], c[3]},
                                        {c[3], c[2]}, {c[2], c[2]}, {c[2], c[1]}, {c[1], c[1]}, {c[1], c[5]}};
    for (int l = 0; l < kUnetLayers; ++l) {
        if (layer_dims[2 * l] != expect[l][0] || layer_dims[2 * l + 1] != expect[l][1]) {
            char msg[160];
            snprintf(msg, sizeof msg, "dpcg_unet_forward: layer %d has weights for %d -> %d channels, the channel list asks for %d -> %d",
                     l, layer_dims[2 * l], layer_dims[2 * l + 1], expect[l][0], expect[l][1]);
            set_error(msg);
            return DPCG_ERR_INVALID;
        }
        if (!weights[l]) return invalid("dpcg_unet_forward: NULL weight");
    }
    if (in_channels != c[0]) {
        char msg[120];
        snprintf(msg, sizeof msg, "dpcg_unet_forward: the input has %d feature channels, enc1 takes %d", in_channels, c[0]);
        set_error(msg);
        return DPCG_ERR_INVALID;
    }
    const int64_t S[kUnetLevels] = {p->lv[0].sites, p->lv[1].sites, p->lv[2].sites, p->lv[3].sites, p->lv[4].sites};
    // buffers: 0..3 = enc1..enc4 (live until their skip), 4 / 5 = scratch
    const int64_t need[6] = {S[0] * c[1], S[1] * c[2], S[2] * c[3], S[3] * c[4],
                             std::max({S[0] * c[1], S[1] * c[2], S[2] * c[3], S[3] * c[4], S[4] * c[5]}),
                             std::max({S[0] * c[1], S[1] * c[2], S[2] * c[3], S[3] * c[4]})};
    for (int b = 0; b < 6; ++b)
        if (p->buf_cap[b] < need[b]) {
            dev_free(p->buf[b]);
            p->buf_cap[b] = 0;
            DPCG_TRY(dev_alloc(&p->buf[b], need[b]));
            p->buf_cap[b] = need[b];
        }
    hipStream_t s = (hipStream_t)stream;
    float *E[4] = {p->buf[0], p->buf[1], p->buf[2], p->buf[3]};
    float *T = p->buf[4], *U = p->buf[5];
    const UnetLevel *lv = p->lv;
    auto conv = [&](int l, int64_t n_out, const int32_t *nbr, const float *in, const float *skip, float *out) {
        unet_conv(expect[l][0], expect[l][1], n_out, nbr, in, weights[l], biases[l], slopes[l], skip, out, s);
    };
    // encoder: enc1 on S0, then (down, enc) per level
    conv(0, S[0], lv[0].subm, features_in, nullptr, E[0]);
    for (int k = 1; k <= 3; ++k) {
        conv(2 * k - 1, S[k], lv[k].down, E[k - 1], nullptr, T);      // down_k: S_k-1 -> S_k
        conv(2 * k, S[k], lv[k].subm, T, nullptr, E[k]);              // enc_k+1
    }
    conv(7, S[4], lv[4].down, E[3], nullptr, T);                      // bottleneck: S3 -> S4
    // decoder: (up + skip, dec) per level, S_k+1 -> S_k
    for (int k = 3; k >= 0; --k) {
        conv(8 + 2 * (3 - k), S[k], lv[k].up, T, E[k], U);            // up3 .. up0
        conv(9 + 2 * (3 - k), S[k], lv[k].subm, U, nullptr, T);       // dec3 .. dec0
    }
    const int32_t *srow = p->site_row, *scol = lv[0].col, *spos = p->lower_pos;
    const float *dec0 = T;
#define DPCG_UNET_OUT(CI)                                                                                                   \
    hipLaunchKernelGGL((k_unet_out_rows<CI>), dim3(grid_blocks(S[0], kConvGrid)), dim3(kBlock), 0, s, S[0], c[5], dec0, weights[16], \
                       biases[16], srow, scol, spos, features_out, lower_val)
    if (c[1] == 16) DPCG_UNET_OUT(16);
    else if (c[1] == 32) DPCG_UNET_OUT(32);
    else if (c[1] == 64) DPCG_UNET_OUT(64);
    else
        hipLaunchKernelGGL(k_unet_out, dim3(grid_blocks(S[0] * c[5], kConvGrid)), dim3(kBlock), 0, s, S[0], c[1], c[5], dec0, weights[16],
                           biases[16], srow, scol, spos, features_out, lower_val);
#undef DPCG_UNET_OUT
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}
