// TemporalGCN (reference neural_dynamics.py:179-238): the LSTM-GNN / GRU-GNN / RNN-GNN baselines of the drivers.  Per tick the
// reference runs a GraphConvolution on an N x 1 column, flattens it to 1 x (N Hg) and feeds an LSTMCell / GRUCell / RNNCell whose input
// weight W_ih is (G Hr) x (N Hg), G = 4 / 3 / 1.  Nothing in the teacher-forced part of that input projection depends on the recurrence,
// so the projections of ALL ticks are one skinny product and W_ih - the only large operand, 4 G Hr Hg bytes per node - is streamed once
// per chunk of ticks instead of once per tick:
//
//   tgcn_proj_f32       GI[tau, g] = b_ih[g] + sum_{i,j} W_ih[g, i Hg + j] relu(S[i, tau] w_j + r_i b_j)        (S = A X, r = A 1)
//   tgcn_proj_bwd_f32   g_Wih, g_w, g_b, g_bih from GGI = dL/dGI: g_Wih written ONCE (no read-modify-write), W_ih read once
//   tgcn_cell_f32       the recurrence over all T ticks in one launch of one workgroup (torch's cell definitions)
//   tgcn_cell_bwd_f32   its reverse (BPTT) in one launch
//
// With input width 1 the graph convolution is Z[i, j] = s_i w_j + r_i b_j: it is formed in registers from the staged S tile, never stored.
// proj uses plain fp32 VALU fma from LDS (not MFMA): the operands of v_mfma_f32_32x32x2f32 would need W_ih rows across lanes, i.e. a gather
// of 4-byte pieces N Hg floats apart or a staged transpose, for a product whose M = G Hr is 10..40 of the 64 rows an MFMA tile pair
// would compute; the staged-slice form below reads W_ih coalesced along its rows and keeps the arithmetic order fixed.
// No floating-point atomics anywhere: per-workgroup partials are summed by a second small launch in a fixed order - same input, same bits.
#include <stdint.h>

#include "common.h"

namespace ndcn {

namespace {

constexpr int kTile = 64;        // nodes per tile: columns [i0 Hg, (i0 + 64) Hg) of every row of W_ih
constexpr int kSlice = 64;       // columns of the tile staged in LDS at a time
constexpr int kMaxM = 64;        // G Hr
constexpr int kMaxHg = 8;
constexpr int kChunk = 80;       // forward: ticks per pass over W_ih (the drivers' 79 training and 80 evaluation ticks are one pass)
constexpr int kChunkB = 32;      // reverse: ticks per staging step; the chunks loop INSIDE a tile's slice, so W_ih is still read once
constexpr int kPad = 84;         // row stride of the forward's S tile and v slice: 16-byte aligned rows, 84 mod 32 = 20 (8 banks of 4 apart)
constexpr int kPer = kChunk / 4; // ticks per wave in the forward
constexpr int kRnn = 0, kGru = 1, kLstm = 2;

int compute_units() {
    static std::atomic<int> cus_of[64];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        cus = cus_of[dev].load(std::memory_order_relaxed);
        if (cus == 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            cus_of[dev].store(cus, std::memory_order_relaxed);
    }
    return cus > 0 ? cus : kCus;
}

inline int64_t n_tiles_of(int64_t N) { return (N + kTile - 1) / kTile; }

// workgroups of the two projection launches: two per compute unit (the forward holds 60 KB of LDS), never more than there are tiles
int proj_grid(int64_t N) {
    const int64_t cap = 2 * (int64_t)compute_units(), t = n_tiles_of(N);
    return (int)(t < cap ? (t < 1 ? 1 : t) : cap);
}

struct ProjArgs {
    const float *S, *r, *w, *b, *Wih;
    float *partial;               // [workgroup][T][M]
    int64_t N, n_tiles;
    int T, Hg, M;
};

// 16 rows of the W_ih slice per wave, one column per lane: 256 contiguous bytes of a row per wave-load, any alignment
__device__ __forceinline__ void load_w(float (&wreg)[16], const float *__restrict__ Wih, int64_t K, int64_t col0, int kt, int s, int M,
                                       int wave, int lane) {
    const int cl = s * kSlice + lane;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int g = wave * 16 + q;
        wreg[q] = (g < M && cl < kt) ? Wih[(int64_t)g * K + col0 + cl] : 0.f;
    }
}

__global__ __launch_bounds__(256) void tgcn_proj_kernel(ProjArgs p) {
    __shared__ __attribute__((aligned(16))) float Sl[kTile][kPad];
    __shared__ __attribute__((aligned(16))) float vl[kSlice][kPad];
    __shared__ float Wl[kMaxM][kSlice + 1];                  // lane = row g in the product: stride 65, conflict-free
    __shared__ float rl[kTile], wl[kMaxHg], bl[kMaxHg];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hg = p.Hg, M = p.M, T = p.T;
    const int64_t K = p.N * Hg;
    if (tid < kMaxHg) {
        wl[tid] = tid < Hg ? p.w[tid] : 0.f;
        bl[tid] = tid < Hg ? p.b[tid] : 0.f;
    }
    for (int tau0 = 0; tau0 < T; tau0 += kChunk) {
        const int tc = T - tau0 < kChunk ? T - tau0 : kChunk;
        float acc[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) acc[q] = 0.f;
        for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
            const int64_t i0 = tile * kTile;
            const int ni = p.N - i0 < kTile ? (int)(p.N - i0) : kTile;
            const int kt = ni * Hg;
            const int64_t col0 = i0 * Hg;
            __syncthreads();                                 // the last tile's readers of Sl / rl / vl / Wl are done
            for (int idx = tid; idx < kTile * kChunk; idx += 256) {
                const int i = idx / kChunk, t = idx - i * kChunk;
                Sl[i][t] = (i < ni && t < tc) ? p.S[(i0 + i) * T + tau0 + t] : 0.f;
            }
            if (tid < kTile) rl[tid] = tid < ni ? p.r[i0 + tid] : 0.f;
            const int n_slices = (kt + kSlice - 1) / kSlice;
            float wreg[16];
            load_w(wreg, p.Wih, K, col0, kt, 0, M, wave, lane);
            for (int s = 0; s < n_slices; ++s) {
                __syncthreads();                             // Sl staged; the last slice's product is done
#pragma unroll
                for (int q = 0; q < 16; ++q) Wl[wave * 16 + q][lane] = wreg[q];
                {
                    // v[k, t] of this slice: thread = (column k = tid / 4, ticks t = 4 q + tid % 4) - one division per slice
                    const int k = tid >> 2, m = tid & 3, cl = s * kSlice + k;
                    const bool valid = cl < kt;
                    const int i = valid ? cl / Hg : 0, j = cl - i * Hg;
                    const float wj = wl[j], rb = rl[i] * bl[j];
#pragma unroll
                    for (int q = 0; q < kPer; ++q) {
                        const int t = 4 * q + m;
                        vl[k][t] = (valid && t < tc) ? relu_nan(fmaf(Sl[i][t], wj, rb)) : 0.f;
                    }
                }
                if (s + 1 < n_slices) load_w(wreg, p.Wih, K, col0, kt, s + 1, M, wave, lane);   // in flight behind the product
                __syncthreads();
#pragma unroll 4
                for (int k = 0; k < kSlice; ++k) {
                    const float wv = Wl[lane][k];
                    const float4 *vp = reinterpret_cast<const float4 *>(&vl[k][wave * kPer]);   // one address per wave: a broadcast
#pragma unroll
                    for (int q4 = 0; q4 < kPer / 4; ++q4) {
                        const float4 v = vp[q4];
                        acc[4 * q4 + 0] = fmaf(wv, v.x, acc[4 * q4 + 0]);
                        acc[4 * q4 + 1] = fmaf(wv, v.y, acc[4 * q4 + 1]);
                        acc[4 * q4 + 2] = fmaf(wv, v.z, acc[4 * q4 + 2]);
                        acc[4 * q4 + 3] = fmaf(wv, v.w, acc[4 * q4 + 3]);
                    }
                }
            }
        }
        if (lane < M) {
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const int t = wave * kPer + q;
                if (t < tc) p.partial[((int64_t)blockIdx.x * T + tau0 + t) * M + lane] = acc[q];
            }
        }
    }
}

// GI = b_ih + the partial blocks in workgroup order
__global__ __launch_bounds__(256) void tgcn_proj_sum_kernel(const float *__restrict__ partial, int nb, int T, int M,
                                                             const float *__restrict__ b_ih, float *__restrict__ GI) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = T * M;
    if (idx >= n) return;
    float s = partial[idx];
    for (int b = 1; b < nb; ++b) s += partial[(int64_t)b * n + idx];
    GI[idx] = s + b_ih[idx % M];
}

struct ProjBwdArgs {
    const float *S, *r, *w, *b, *Wih, *GG;
    float *gWih;
    double *partial;              // [workgroup][2 kMaxHg]: g_w then g_b
    int64_t N, n_tiles;
    int T, Hg, M;
};

__global__ __launch_bounds__(256) void tgcn_proj_bwd_kernel(ProjBwdArgs p) {
    __shared__ float Sl[kTile][kChunkB + 1];                              // lanes differ in i: stride 33
    __shared__ float vl[kChunkB][kSlice];                                 // [tick][column]: lane = column
    __shared__ float Wl[kMaxM][kSlice];                                   // [g][column]
    __shared__ __attribute__((aligned(16))) float GGl[kChunkB][kMaxM];    // [tick][g]
    __shared__ __attribute__((aligned(16))) double GGt[kMaxM][kChunkB];   // [g][tick], widened once: gZ and its two sums are formed in fp64
    __shared__ float rl[kTile], wl[kMaxHg], bl[kMaxHg];
    __shared__ double red[4][2 * kMaxHg];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hg = p.Hg, M = p.M, T = p.T;
    const int64_t K = p.N * Hg;
    if (tid < kMaxHg) {
        wl[tid] = tid < Hg ? p.w[tid] : 0.f;
        bl[tid] = tid < Hg ? p.b[tid] : 0.f;
    }
    double pw[kMaxHg], pb[kMaxHg];
#pragma unroll
    for (int j = 0; j < kMaxHg; ++j) pw[j] = pb[j] = 0.0;
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * kTile;
        const int ni = p.N - i0 < kTile ? (int)(p.N - i0) : kTile;
        const int kt = ni * Hg;
        const int64_t col0 = i0 * Hg;
        __syncthreads();                                     // the last tile's readers of rl are done
        if (tid < kTile) rl[tid] = tid < ni ? p.r[i0 + tid] : 0.f;
        const int n_slices = (kt + kSlice - 1) / kSlice;
        for (int s = 0; s < n_slices; ++s) {
            const int cl = s * kSlice + lane;
            const bool valid = cl < kt;
            const int i = valid ? cl / Hg : 0, j = cl - i * Hg;
            __syncthreads();                                 // the last slice's readers of Wl are done
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int g = wave * 16 + q;
                Wl[g][lane] = (g < M && valid) ? p.Wih[(int64_t)g * K + col0 + cl] : 0.f;
            }
            float accW[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) accW[q] = 0.f;
            double sw = 0.0, sb = 0.0;
            for (int tau0 = 0; tau0 < T; tau0 += kChunkB) {
                const int tc = T - tau0 < kChunkB ? T - tau0 : kChunkB;
                __syncthreads();                             // the last chunk's readers of Sl / vl / GGl / GGt are done
                for (int idx = tid; idx < kTile * kChunkB; idx += 256) {
                    const int ii = idx / kChunkB, t = idx % kChunkB;
                    Sl[ii][t] = (ii < ni && t < tc) ? p.S[(i0 + ii) * T + tau0 + t] : 0.f;
                }
                for (int idx = tid; idx < kChunkB * kMaxM; idx += 256) {
                    const int t = idx / kMaxM, g = idx % kMaxM;
                    const float x = (t < tc && g < M) ? p.GG[(int64_t)(tau0 + t) * M + g] : 0.f;
                    GGl[t][g] = x;
                    GGt[g][t] = (double)x;
                }
                __syncthreads();
                {
                    const float wj = wl[j], rb = rl[i] * bl[j];
#pragma unroll
                    for (int q = 0; q < kChunkB / 4; ++q) {
                        const int t = wave * (kChunkB / 4) + q;
                        vl[t][lane] = (valid && t < tc) ? relu_nan(fmaf(Sl[i][t], wj, rb)) : 0.f;
                    }
                }
                __syncthreads();
                // g_Wih[g, column] += sum_t GGI[t, g] v[column, t]: this thread's 16 rows g of its column
                for (int t = 0; t < kChunkB; ++t) {
                    const float vv = vl[t][lane];
                    const float4 *gp = reinterpret_cast<const float4 *>(&GGl[t][wave * 16]);
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const float4 gg = gp[q4];
                        accW[4 * q4 + 0] = fmaf(gg.x, vv, accW[4 * q4 + 0]);
                        accW[4 * q4 + 1] = fmaf(gg.y, vv, accW[4 * q4 + 1]);
                        accW[4 * q4 + 2] = fmaf(gg.z, vv, accW[4 * q4 + 2]);
                        accW[4 * q4 + 3] = fmaf(gg.w, vv, accW[4 * q4 + 3]);
                    }
                }
                // gZ[column, t] = [Z > 0] sum_g W_ih[g, column] GGI[t, g]: this thread's 8 ticks of its column.  In fp64 (every product of
                // two floats is exact there): g_w and g_b are sums of N T signed terms each, where fp32 terms leave only what the
                // cancellation spares; v_fma_f64 issues at the rate of the unpacked v_fma_f32
                double az[kChunkB / 4];
#pragma unroll
                for (int q = 0; q < kChunkB / 4; ++q) az[q] = 0.0;
                for (int g = 0; g < M; ++g) {
                    const double wv = (double)Wl[g][lane];
                    const double2 *gp = reinterpret_cast<const double2 *>(&GGt[g][wave * (kChunkB / 4)]);
#pragma unroll
                    for (int q2 = 0; q2 < kChunkB / 8; ++q2) {
                        const double2 a = gp[q2];
                        az[2 * q2 + 0] = fma(wv, a.x, az[2 * q2 + 0]);
                        az[2 * q2 + 1] = fma(wv, a.y, az[2 * q2 + 1]);
                    }
                }
#pragma unroll
                for (int q = 0; q < kChunkB / 4; ++q) {
                    const int t = wave * (kChunkB / 4) + q;
                    const float vv = vl[t][lane];
                    const double gz = vv <= 0.f ? 0.0 : az[q];           // 0 at Z = 0; a NaN output passes the gradient
                    sw = fma(gz, (double)Sl[i][t], sw);
                    sb += gz;
                }
            }
            if (valid) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int g = wave * 16 + q;
                    if (g < M) p.gWih[(int64_t)g * K + col0 + cl] = accW[q];
                }
            }
            sb *= (double)rl[i];
#pragma unroll
            for (int jj = 0; jj < kMaxHg; ++jj) {
                if (valid && j == jj) { pw[jj] += sw; pb[jj] += sb; }
            }
        }
    }
    // the workgroup's g_w / g_b: lanes by a fixed shuffle tree, then the four waves in order
#pragma unroll
    for (int jj = 0; jj < kMaxHg; ++jj) {
        double a = pw[jj], b = pb[jj];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64);
            b += __shfl_down(b, off, 64);
        }
        if (lane == 0) { red[wave][jj] = a; red[wave][kMaxHg + jj] = b; }
    }
    __syncthreads();
    if (tid < 2 * kMaxHg) p.partial[(int64_t)blockIdx.x * 2 * kMaxHg + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// g_w, g_b: the workgroups' partials in fp64, in workgroup order; g_bih: the column sums of GGI in fp64, in tick order
__global__ __launch_bounds__(128) void tgcn_proj_bwd_finish_kernel(const double *__restrict__ partial, int nb, const float *__restrict__ GG,
                                                                    int T, int Hg, int M, float *__restrict__ g_w, float *__restrict__ g_b,
                                                                    float *__restrict__ g_bih) {
    const int tid = threadIdx.x;
    if (tid < 2 * kMaxHg) {
        const int j = tid % kMaxHg;
        if (j < Hg) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += partial[(int64_t)b * 2 * kMaxHg + tid];
            (tid < kMaxHg ? g_w : g_b)[j] = (float)s;
        }
    } else if (tid >= 64 && tid - 64 < M) {
        const int g = tid - 64;
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += (double)GG[(int64_t)t * M + g];
        g_bih[g] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ the recurrence
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

struct CellArgs {
    const float *GI, *Whh, *bhh, *h0, *c0;
    float *H, *gates, *crec, *hT, *cT;
    int T, Hr, type;
};

// One wave: thread g < M owns row g of W_hh h + b_hh, thread k < Hr owns element k of the state.  The record per tick (4 Hr floats):
// lstm i, f, g, o; gru r, z, n and W_hn h + b_hn; rnn h' - what the reverse reads instead of re-forming it.
__global__ __launch_bounds__(64) void tgcn_cell_kernel(CellArgs p) {
    __shared__ float Wl[kMaxM][kMaxM + 1];
    __shared__ float hl[kMaxM], pre[kMaxM], ghl[kMaxM];
    const int g = threadIdx.x, Hr = p.Hr, type = p.type;
    const int M = (type == kLstm ? 4 : type == kGru ? 3 : 1) * Hr;
    for (int idx = g; idx < M * Hr; idx += 64) Wl[idx / Hr][idx % Hr] = p.Whh[idx];
    const float bh = g < M ? p.bhh[g] : 0.f;
    float c = 0.f, hn = 0.f;
    if (g < Hr) {
        hn = p.h0 ? p.h0[g] : 0.f;
        hl[g] = hn;
        c = (type == kLstm && p.c0) ? p.c0[g] : 0.f;
    }
    __syncthreads();
    for (int tau = 0; tau < p.T; ++tau) {
        float gh = bh;
        if (g < M) {
            for (int k = 0; k < Hr; ++k) gh = fmaf(Wl[g][k], hl[k], gh);
            const float gi = p.GI[(int64_t)tau * M + g];
            pre[g] = (type == kGru && g >= 2 * Hr) ? gi : gi + gh;
            ghl[g] = gh;
        }
        __syncthreads();
        if (g < Hr) {
            float *rec = p.gates + (int64_t)tau * 4 * Hr;
            if (type == kLstm) {
                const float i = sigm(pre[g]), f = sigm(pre[Hr + g]), gg = tanhf(pre[2 * Hr + g]), o = sigm(pre[3 * Hr + g]);
                c = f * c + i * gg;
                hn = o * tanhf(c);
                rec[g] = i; rec[Hr + g] = f; rec[2 * Hr + g] = gg; rec[3 * Hr + g] = o;
                p.crec[(int64_t)tau * Hr + g] = c;
            } else if (type == kGru) {
                const float r = sigm(pre[g]), z = sigm(pre[Hr + g]), hv = ghl[2 * Hr + g];
                const float n = tanhf(pre[2 * Hr + g] + r * hv);
                hn = (1.f - z) * n + z * hl[g];
                rec[g] = r; rec[Hr + g] = z; rec[2 * Hr + g] = n; rec[3 * Hr + g] = hv;
            } else {
                hn = tanhf(pre[g]);
                rec[g] = hn;
            }
            p.H[(int64_t)tau * Hr + g] = hn;
            hl[g] = hn;                                      // every read of hl by another thread was before the barrier above
        }
        __syncthreads();
    }
    if (g < Hr) {
        if (p.hT) p.hT[g] = hn;
        if (p.cT && type == kLstm) p.cT[g] = c;
    }
}

struct CellBwdArgs {
    const float *gH, *gates, *crec, *Hrec, *h0, *c0, *Whh;
    float *GG, *gWhh, *gbhh, *gh0, *gc0;
    int T, Hr, type;
};

__global__ __launch_bounds__(256) void tgcn_cell_bwd_kernel(CellBwdArgs p) {
    __shared__ float Wl[kMaxM][kMaxM + 1];
    __shared__ double gWl[kMaxM * kMaxM];                    // g_Whh in fp64, every element owned by one thread
    __shared__ float dal[kMaxM], hpl[kMaxM];
    const int tid = threadIdx.x, Hr = p.Hr, type = p.type;
    const int M = (type == kLstm ? 4 : type == kGru ? 3 : 1) * Hr;
    for (int e = tid; e < M * Hr; e += 256) {
        Wl[e / Hr][e % Hr] = p.Whh[e];
        gWl[e] = 0.0;
    }
    float dc = 0.f, dh_next = 0.f, direct = 0.f;
    double gb = 0.0;
    __syncthreads();
    for (int tau = p.T - 1; tau >= 0; --tau) {
        if (tid < Hr) {
            const int k = tid;
            const float hprev = tau > 0 ? p.Hrec[(int64_t)(tau - 1) * Hr + k] : (p.h0 ? p.h0[k] : 0.f);
            hpl[k] = hprev;
            const float dh = p.gH[(int64_t)tau * Hr + k] + dh_next;
            const float *rec = p.gates + (int64_t)tau * 4 * Hr;
            float *gg_out = p.GG + (int64_t)tau * M;
            if (type == kLstm) {
                const float i = rec[k], f = rec[Hr + k], gg = rec[2 * Hr + k], o = rec[3 * Hr + k];
                const float cprev = tau > 0 ? p.crec[(int64_t)(tau - 1) * Hr + k] : (p.c0 ? p.c0[k] : 0.f);
                const float tc = tanhf(p.crec[(int64_t)tau * Hr + k]);
                const float dcc = dc + dh * o * (1.f - tc * tc);
                const float dai = dcc * gg * i * (1.f - i), daf = dcc * cprev * f * (1.f - f);
                const float dag = dcc * i * (1.f - gg * gg), dao = dh * tc * o * (1.f - o);
                dc = dcc * f;
                gg_out[k] = dai; gg_out[Hr + k] = daf; gg_out[2 * Hr + k] = dag; gg_out[3 * Hr + k] = dao;
                dal[k] = dai; dal[Hr + k] = daf; dal[2 * Hr + k] = dag; dal[3 * Hr + k] = dao;
                direct = 0.f;
            } else if (type == kGru) {
                const float r = rec[k], z = rec[Hr + k], n = rec[2 * Hr + k], hv = rec[3 * Hr + k];
                const float dan = dh * (1.f - z) * (1.f - n * n);
                const float dar = dan * hv * r * (1.f - r), daz = dh * (hprev - n) * z * (1.f - z);
                gg_out[k] = dar; gg_out[Hr + k] = daz; gg_out[2 * Hr + k] = dan;
                dal[k] = dar; dal[Hr + k] = daz; dal[2 * Hr + k] = dan * r;
                direct = dh * z;
            } else {
                const float h = p.Hrec[(int64_t)tau * Hr + k];
                const float da = dh * (1.f - h * h);
                gg_out[k] = da;
                dal[k] = da;
                direct = 0.f;
            }
        }
        __syncthreads();
        if (tid < Hr) {
            float s = direct;
            for (int g = 0; g < M; ++g) s = fmaf(Wl[g][tid], dal[g], s);
            dh_next = s;
        }
        if (tid < M) gb += (double)dal[tid];
        for (int e = tid; e < M * Hr; e += 256) gWl[e] = fma((double)dal[e / Hr], (double)hpl[e % Hr], gWl[e]);
        __syncthreads();                                     // before the next tick overwrites dal / hpl
    }
    for (int e = tid; e < M * Hr; e += 256) p.gWhh[e] = (float)gWl[e];
    if (tid < M) p.gbhh[tid] = (float)gb;
    if (tid < Hr) {
        if (p.gh0) p.gh0[tid] = dh_next;
        if (p.gc0 && type == kLstm) p.gc0[tid] = dc;
    }
}

int gates_of(int type) { return type == kLstm ? 4 : type == kGru ? 3 : type == kRnn ? 1 : 0; }

int check_proj_shape(const char *who, int64_t N, int T, int Hg, int M) {
    if (N < 1 || T < 1 || (int64_t)T * kMaxM > INT_MAX / 4) { set_error("%s: N = %lld, T = %d (both >= 1)", who, (long long)N, T); return NDCN_EINVAL; }
    if (Hg < 1 || Hg > kMaxHg) { set_error("%s: hidden_size_gnn = %d, the kernel takes 1..%d", who, Hg, kMaxHg); return NDCN_EINVAL; }
    if (M < 1 || M > kMaxM) { set_error("%s: G * hidden_size_rnn = %d, the kernel takes 1..%d", who, M, kMaxM); return NDCN_EINVAL; }
    return NDCN_OK;
}

}  // namespace

int64_t tgcn_proj_ws_bytes(int64_t N, int T, int M) {
    if (N < 1 || T < 1 || M < 1) return 0;
    return (int64_t)proj_grid(N) * T * M * (int64_t)sizeof(float);
}

int tgcn_proj_f32(const float *S, const float *r, const float *w, const float *b, const float *Wih, const float *bih, float *GI, void *ws,
                  int64_t N, int T, int Hg, int M, hipStream_t st) {
    int rc = check_proj_shape("tgcn_proj", N, T, Hg, M);
    if (rc) return rc;
    if (!S || !r || !w || !b || !Wih || !bih || !GI || !ws) { set_error("tgcn_proj: null argument"); return NDCN_EINVAL; }
    if (GI == S || GI == r || GI == w || GI == b || GI == Wih || GI == bih || ws == (const void *)S || ws == (const void *)r ||
        ws == (const void *)Wih || ws == (const void *)GI) {
        set_error("tgcn_proj: GI or the workspace aliases an input");
        return NDCN_EINVAL;
    }
    ProjArgs p;
    p.S = S; p.r = r; p.w = w; p.b = b; p.Wih = Wih;
    p.partial = static_cast<float *>(ws);
    p.N = N; p.n_tiles = n_tiles_of(N);
    p.T = T; p.Hg = Hg; p.M = M;
    const int grid = proj_grid(N);
    hipLaunchKernelGGL(tgcn_proj_kernel, dim3(grid), dim3(256), 0, st, p);
    NDCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(tgcn_proj_sum_kernel, dim3((T * M + 255) / 256), dim3(256), 0, st, p.partial, grid, T, M, bih, GI);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int64_t tgcn_proj_bwd_ws_bytes(int64_t N) {
    if (N < 1) return 0;
    return (int64_t)proj_grid(N) * 2 * kMaxHg * (int64_t)sizeof(double);
}

int tgcn_proj_bwd_f32(const float *S, const float *r, const float *w, const float *b, const float *Wih, const float *GG, float *gWih,
                      float *gw, float *gb, float *gbih, void *ws, int64_t N, int T, int Hg, int M, hipStream_t st) {
    int rc = check_proj_shape("tgcn_proj_bwd", N, T, Hg, M);
    if (rc) return rc;
    if (!S || !r || !w || !b || !Wih || !GG || !gWih || !gw || !gb || !gbih || !ws) { set_error("tgcn_proj_bwd: null argument"); return NDCN_EINVAL; }
    const void *ins[] = {S, r, w, b, Wih, GG};
    void *outs[] = {gWih, gw, gb, gbih, ws};
    for (int o = 0; o < 5; ++o) {
        for (int i = 0; i < 6; ++i)
            if (outs[o] == ins[i]) { set_error("tgcn_proj_bwd: an output aliases an input (g_Wih is written, never accumulated)"); return NDCN_EINVAL; }
        for (int q = 0; q < o; ++q)
            if (outs[o] == outs[q]) { set_error("tgcn_proj_bwd: two outputs alias"); return NDCN_EINVAL; }
    }
    ProjBwdArgs p;
    p.S = S; p.r = r; p.w = w; p.b = b; p.Wih = Wih; p.GG = GG;
    p.gWih = gWih;
    p.partial = static_cast<double *>(ws);
    p.N = N; p.n_tiles = n_tiles_of(N);
    p.T = T; p.Hg = Hg; p.M = M;
    const int grid = proj_grid(N);
    hipLaunchKernelGGL(tgcn_proj_bwd_kernel, dim3(grid), dim3(256), 0, st, p);
    NDCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(tgcn_proj_bwd_finish_kernel, dim3(1), dim3(128), 0, st, p.partial, grid, GG, T, Hg, M, gw, gb, gbih);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int tgcn_cell_f32(int type, const float *GI, const float *Whh, const float *bhh, const float *h0, const float *c0, float *H, float *gates,
                  float *crec, float *hT, float *cT, int T, int Hr, hipStream_t st) {
    const int G = gates_of(type);
    if (G == 0) { set_error("tgcn_cell: rnn_type %d (0 rnn, 1 gru, 2 lstm)", type); return NDCN_EINVAL; }
    if (Hr < 1 || G * Hr > kMaxM) { set_error("tgcn_cell: G * hidden_size_rnn = %d, the kernel takes 1..%d", G * Hr, kMaxM); return NDCN_EINVAL; }
    if (T < 1) { set_error("tgcn_cell: T = %d", T); return NDCN_EINVAL; }
    if (!GI || !Whh || !bhh || !H || !gates || (type == kLstm && !crec)) { set_error("tgcn_cell: null argument"); return NDCN_EINVAL; }
    const void *ins[] = {GI, Whh, bhh, h0, c0};
    void *outs[] = {H, gates, crec, hT, cT};
    for (int o = 0; o < 5; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 5; ++i)
            if (outs[o] == ins[i]) { set_error("tgcn_cell: an output aliases an input"); return NDCN_EINVAL; }
        for (int q = 0; q < o; ++q)
            if (outs[o] == outs[q]) { set_error("tgcn_cell: two outputs alias"); return NDCN_EINVAL; }
    }
    CellArgs p;
    p.GI = GI; p.Whh = Whh; p.bhh = bhh; p.h0 = h0; p.c0 = c0;
    p.H = H; p.gates = gates; p.crec = crec; p.hT = hT; p.cT = cT;
    p.T = T; p.Hr = Hr; p.type = type;
    hipLaunchKernelGGL(tgcn_cell_kernel, dim3(1), dim3(64), 0, st, p);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int tgcn_cell_bwd_f32(int type, const float *gH, const float *gates, const float *crec, const float *Hrec, const float *h0, const float *c0,
                      const float *Whh, float *GG, float *gWhh, float *gbhh, float *gh0, float *gc0, int T, int Hr, hipStream_t st) {
    const int G = gates_of(type);
    if (G == 0) { set_error("tgcn_cell_bwd: rnn_type %d (0 rnn, 1 gru, 2 lstm)", type); return NDCN_EINVAL; }
    if (Hr < 1 || G * Hr > kMaxM) { set_error("tgcn_cell_bwd: G * hidden_size_rnn = %d, the kernel takes 1..%d", G * Hr, kMaxM); return NDCN_EINVAL; }
    if (T < 1) { set_error("tgcn_cell_bwd: T = %d", T); return NDCN_EINVAL; }
    if (!gH || !gates || !Hrec || !Whh || !GG || !gWhh || !gbhh || (type == kLstm && !crec)) { set_error("tgcn_cell_bwd: null argument"); return NDCN_EINVAL; }
    const void *ins[] = {gH, gates, crec, Hrec, h0, c0, Whh};
    void *outs[] = {GG, gWhh, gbhh, gh0, gc0};
    for (int o = 0; o < 5; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 7; ++i)
            if (outs[o] == ins[i]) { set_error("tgcn_cell_bwd: an output aliases an input"); return NDCN_EINVAL; }
        for (int q = 0; q < o; ++q)
            if (outs[o] == outs[q]) { set_error("tgcn_cell_bwd: two outputs alias"); return NDCN_EINVAL; }
    }
    CellBwdArgs p;
    p.gH = gH; p.gates = gates; p.crec = crec; p.Hrec = Hrec; p.h0 = h0; p.c0 = c0; p.Whh = Whh;
    p.GG = GG; p.gWhh = gWhh; p.gbhh = gbhh; p.gh0 = gh0; p.gc0 = gc0;
    p.T = T; p.Hr = Hr; p.type = type;
    hipLaunchKernelGGL(tgcn_cell_bwd_kernel, dim3(1), dim3(256), 0, st, p);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn

using namespace ndcn;

extern "C" {

int ndcn_tgcn_chunk(int reverse) { return reverse ? kChunkB : kChunk; }

int64_t ndcn_tgcn_proj_ws_bytes(int64_t n_nodes, int T, int M) { return tgcn_proj_ws_bytes(n_nodes, T, M); }

int ndcn_tgcn_proj_f32(const float *S, const float *r, const float *w, const float *b, const float *W_ih, const float *b_ih, float *GI,
                       void *ws, int64_t n_nodes, int T, int Hg, int M, void *stream) {
    return tgcn_proj_f32(S, r, w, b, W_ih, b_ih, GI, ws, n_nodes, T, Hg, M, static_cast<hipStream_t>(stream));
}

int64_t ndcn_tgcn_proj_bwd_ws_bytes(int64_t n_nodes) { return tgcn_proj_bwd_ws_bytes(n_nodes); }

int ndcn_tgcn_proj_bwd_f32(const float *S, const float *r, const float *w, const float *b, const float *W_ih, const float *GGI,
                           float *g_Wih, float *g_w, float *g_b, float *g_bih, void *ws, int64_t n_nodes, int T, int Hg, int M,
                           void *stream) {
    return tgcn_proj_bwd_f32(S, r, w, b, W_ih, GGI, g_Wih, g_w, g_b, g_bih, ws, n_nodes, T, Hg, M, static_cast<hipStream_t>(stream));
}

int ndcn_tgcn_cell_f32(int rnn_type, const float *GI, const float *W_hh, const float *b_hh, const float *h0, const float *c0, float *H,
                       float *gates, float *c_rec, float *hT, float *cT, int T, int Hr, void *stream) {
    return tgcn_cell_f32(rnn_type, GI, W_hh, b_hh, h0, c0, H, gates, c_rec, hT, cT, T, Hr, static_cast<hipStream_t>(stream));
}

int ndcn_tgcn_cell_bwd_f32(int rnn_type, const float *gH, const float *gates, const float *c_rec, const float *H, const float *h0,
                           const float *c0, const float *W_hh, float *GGI, float *g_Whh, float *g_bhh, float *g_h0, float *g_c0, int T,
                           int Hr, void *stream) {
    return tgcn_cell_bwd_f32(rnn_type, gH, gates, c_rec, H, h0, c0, W_hh, GGI, g_Whh, g_bhh, g_h0, g_c0, T, Hr,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
