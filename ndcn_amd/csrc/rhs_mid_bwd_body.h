// The body of rhs_mid_bwd_kernel (rhs_mid_bwd.hip), included once per kernel: the text between the braces, with the kernel's argument
// struct `a` in scope.  MB_GS_STORE(v) is what the gS store writes for the accumulator element v: v itself in rhs_mid_bwd_kernel - whose
// token stream, and so whose device code, is what it was before this file existed - and alpha * v (one rounding: scale_kernel's w * x)
// in rhs_mid_bwd_scaled_kernel, the no_graph ablation's gX = alpha gZ W without the scaling pass (rhs_abl_bwd.hip).  No include guard:
// it is meant to be included twice.
    extern __shared__ __align__(16) float mb_lds[];
    const int H = a.H;
    const int P = (H + 31) & ~31;
    const int ld = P + 1;                                    // odd leading dimension: the column-ish operand reads are conflict-free
    const int H4 = H >> 2, P4 = P >> 2;
    float *s_W = mb_lds;                                     // [P][ld]  s_W[o * ld + i] = W[o][i], zero beyond H
    float *s_S = mb_lds + P * ld;                            // [64][ld] the S tile
    float *s_G = s_S + kMbTile * ld;                         // [64][ld] the gZ tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kk = lane >> 5;
    for (int i = tid; i < P * P; i += kMbThreads) {
        const int o = i / P, k = i - o * P;
        s_W[o * ld + k] = (o < H && k < H) ? a.W[o * H + k] : 0.f;
    }
    const int r_lo = (int)blockIdx.x * a.rpc;                // (n_rows < 2^31 - 64: the launcher's check)
    const int r_hi = a.n_rows - r_lo < a.rpc ? a.n_rows : r_lo + a.rpc;
    // gather roles (rhs_mid.hip)
    const int lsh = a.lsh;
    const int gr_row = tid >> lsh, c4 = (tid & ((1 << lsh) - 1)) * 4, rows_per_pass = kMbThreads >> lsh;
    const bool act = c4 < H, pad = c4 < P;
    // gS roles
    const int nI = P >> 5;
    const int wm = wave & 1, tn = wave >> 1;
    const bool gs_job = a.gS && wave < 2 * nI;
    // gW roles: pair p = (o-strip p / nI, i-tile p % nI); this wave's pairs are `wave` and `wave + 8`
    const int n_pairs = nI * nI;
    const bool job0 = wave < n_pairs, job1 = wave + 8 < n_pairs;
    const int os0 = wave / nI, it0 = wave - os0 * nI;
    const int os1 = (wave + 8) / nI, it1 = (wave + 8) - os1 * nI;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = 0.f, acc1[i] = 0.f;
    float bsum0 = 0.f, bsum1 = 0.f;
    for (int r0 = r_lo; r0 < r_hi; r0 += kMbTile) {
        const int rows = r_hi - r0 < kMbTile ? r_hi - r0 : kMbTile;
        // ---- S tile
        if (a.S) {
            for (int i = tid; i < kMbTile * P4; i += kMbThreads) {
                const int row = i / P4, q = i - row * P4;
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < rows && q < H4) s = mb_ld4(a.S + (size_t)(r0 + row) * H + 4 * q);
                float *d = s_S + row * ld + 4 * q;
                d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w;
            }
        } else {
            for (int row = gr_row; row < kMbTile; row += rows_per_pass) {
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < rows && act) {
                    int j = a.rowptr[r0 + row];
                    const int j1 = a.rowptr[r0 + row + 1];
                    const float *xc = a.X + c4;
                    for (; j + 4 <= j1; j += 4) {
                        const int q0 = a.colidx[j], q1 = a.colidx[j + 1], q2 = a.colidx[j + 2], q3 = a.colidx[j + 3];
                        const float v0 = a.val[j], v1 = a.val[j + 1], v2 = a.val[j + 2], v3 = a.val[j + 3];
                        const float4 x0 = mb_ld4(xc + (size_t)q0 * H), x1 = mb_ld4(xc + (size_t)q1 * H);
                        const float4 x2 = mb_ld4(xc + (size_t)q2 * H), x3 = mb_ld4(xc + (size_t)q3 * H);
                        mb_fma4(s, v0, x0); mb_fma4(s, v1, x1); mb_fma4(s, v2, x2); mb_fma4(s, v3, x3);
                    }
                    for (; j < j1; ++j) mb_fma4(s, a.val[j], mb_ld4(xc + (size_t)a.colidx[j] * H));
                }
                if (pad) {
                    float *d = s_S + row * ld + c4;
                    d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w;
                }
            }
        }
        // ---- gZ tile
        for (int i = tid; i < kMbTile * P4; i += kMbThreads) {
            const int row = i / P4, q = i - row * P4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < rows && q < H4) {
                const size_t idx = (size_t)(r0 + row) * H + 4 * q;
                v = mb_ld4(a.g + idx);
                if (a.K) {
                    const float4 k = mb_ld4(a.K + idx);
                    v.x = mb_mask(v.x, k.x); v.y = mb_mask(v.y, k.y); v.z = mb_mask(v.z, k.z); v.w = mb_mask(v.w, k.w);
                }
            }
            float *d = s_G + row * ld + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
        // ---- gS = gZ W: one 32 x 32 output tile per wave, k = o ascending from a zero accumulator (linear_gs_kernel)
        if (gs_job && wm * 32 < rows) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            const float *pa = s_G + (wm * 32 + l31) * ld + kk;
            const float *pb = s_W + kk * ld + tn * 32 + l31;
            for (int k0 = 0; k0 < P; k0 += 32)
#pragma unroll
                for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k0 + k], pb[(k0 + k) * ld], acc, 0, 0, 0);
            const int col = tn * 32 + l31;
            if (col < H) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                    if (m < rows) a.gS[(size_t)(r0 + m) * H + col] = MB_GS_STORE(acc[r]);
                }
            }
        }
        // ---- gW, gb: row pairs ascending, whole rounds of 8 rows as linear_wgrad_kernel walks them
        if (job0) {
            const int n_u = ((rows + 7) & ~7) >> 1;
            const float *pa0 = s_G + kk * ld + os0 * 32 + l31, *pb0 = s_S + kk * ld + it0 * 32 + l31;
            const float *pa1 = s_G + kk * ld + os1 * 32 + l31, *pb1 = s_S + kk * ld + it1 * 32 + l31;
            if (job1) {
                for (int u = 0; u < n_u; ++u) {
                    const float a0 = pa0[2 * u * ld], b0 = pb0[2 * u * ld], a1 = pa1[2 * u * ld], b1 = pb1[2 * u * ld];
                    bsum0 += a0;
                    bsum1 += a1;
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc1, 0, 0, 0);
                }
            } else {
                for (int u = 0; u < n_u; ++u) {
                    const float a0 = pa0[2 * u * ld], b0 = pb0[2 * u * ld];
                    bsum0 += a0;
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
                }
            }
        }
        __syncthreads();                                     // the next tile's loads overwrite both tiles
    }
    // ---- the chunk's partial block and bias row (linear_wgrad_kernel's layout)
    float *pw = a.part_w + (size_t)blockIdx.x * H * H;
    if (job0) {
        const int i = it0 * 32 + l31;
        if (i < H) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int oo = os0 * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * kk;
                if (oo < H) pw[(size_t)oo * H + i] = acc0[rr];
            }
        }
        if (a.part_b && it0 == 0) {
            bsum0 += __shfl_xor(bsum0, 32, 64);              // the two row parities of this column
            const int o = os0 * 32 + l31;
            if (lane < 32 && o < H) a.part_b[(size_t)blockIdx.x * H + o] = bsum0;
        }
    }
    if (job1) {
        const int i = it1 * 32 + l31;
        if (i < H) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int oo = os1 * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * kk;
                if (oo < H) pw[(size_t)oo * H + i] = acc1[rr];
            }
        }
        if (a.part_b && it1 == 0) {
            bsum1 += __shfl_xor(bsum1, 32, 64);
            const int o = os1 * 32 + l31;
            if (lane < 32 && o < H) a.part_b[(size_t)blockIdx.x * H + o] = bsum1;
        }
    }
