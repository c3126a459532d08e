// Body shared by small_finish_kernel and small_finish_batch_kernel (small.hip includes it into both): `a` is the lane's argument struct.
  extern __shared__ __attribute__((aligned(16))) double small_lds[];
  double* const Ui = small_lds;        // [SM][SLD] U^-1
  double* const Ri = Ui + SM * SLD;    // [SM][SLD] R~^-1
  double* const Wt = Ri + SM * SLD;    // [SM][SLD] W~, then W
  double* const Yt = Wt + SM * SLD;    // [SM][SLD] W~ U^-T
  double* const zs = Yt + SM * SLD;    // [SM][DT]
  double* const tt = zs + SM * DT;     // [SM]
  double* const red = tt + SM;         // [4][SM]
  double* const msL = red + 4 * SM;    // MS: [SM][DT] multiscales (padding 1)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int d = a.d, m = a.m;
  load_corner(a.uinv, a.mp, Ui, tid);
  load_corner(a.rinv, a.mp, Ri, tid);
  if (tid < SM) tt[tid] = a.ttil[tid];
  for (int idx = tid; idx < SM * DT; idx += 256) {
    const int c = idx / DT, k = idx % DT;
    zs[idx] = (k < d && c < m) ? a.Z[(int64_t)c * d + k] : 0.0;
    if constexpr (MS) msL[idx] = (k < d && c < m) ? a.ms[(int64_t)c * d + k] : 1.0;
  }
  for (int64_t i = tid; i < a.n_gather; i += 256) a.ex[i] = a.gather_from[i];
  double kreg[16];  // K_m entries of the trace phase below (thread = column, group of 16 rows): loaded now, used at the end
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = (tid >> 6) * 16 + i;
    kreg[i] = (r < m && lane < m) ? a.km[(int64_t)r * a.mp + lane] : 0.0;
  }
  __syncthreads();
  sd4 acc[4];
  rows_times<true>(Ri, Ri, wv, l15, lq, acc);  // B~^-1
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * wv + lq + 4 * r;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int c = 16 * ct + l15;
      const int rr = min(row, c), cc = max(row, c);  // G~ is valid in the upper triangle: mirrored, as build_w_kernel
      Wt[row * SLD + c] = (row == c ? 1.0 : 0.0) - acc[ct][r] - tt[row] * tt[c] - a.g[rr * TILE + cc];
    }
  }
  rows_times<true>(Wt, Ui, wv, l15, lq, acc);  // Y = W~ U^-T (rows of this wavefront)
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) Yt[(16 * wv + lq + 4 * r) * SLD + 16 * ct + l15] = acc[ct][r];
  __syncthreads();
  rows_times<false>(Ui, Yt, wv, l15, lq, acc);  // W = U^-1 Y
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * wv + lq + 4 * r;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      Wt[row * SLD + 16 * ct + l15] = acc[ct][r];
      a.wmat[(int64_t)row * a.mp + 16 * ct + l15] = acc[ct][r];
    }
  }
  __syncthreads();
  const int col = lane, rg = wv;
  double g[DT], gm[MS ? DT : 1], s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int k = 0; k < DT; ++k) g[k] = 0.0;
  if constexpr (MS) {
#pragma unroll
    for (int k = 0; k < DT; ++k) gm[k] = 0.0;
  }
  if (col < m) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = rg * 16 + i;
      const double wk = Wt[r * SLD + col] * kreg[i];  // (0 beyond the real rows)
      s0 += wk;
      if constexpr (MS) {
        if (r != col) {
#pragma unroll
          for (int k = 0; k < DT; ++k) {
            if (k < d) {
              const double iscale = 1.0 / ((msL[r * DT + k] + msL[col * DT + k]) - 1.0);
              const double sdiff = (zs[r * DT + k] - zs[col * DT + k]) * iscale;
              g[k] += wk * sdiff;
              gm[k] += wk * (iscale - sdiff * sdiff);
            }
          }
        }
      } else {
        double dist = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k) {
          const double df = zs[r * DT + k] - zs[col * DT + k];
          dist += df * df;
          g[k] += wk * df;
        }
        s1 += wk * dist;
      }
    }
  }
  for (int q = 0; q < a.km_rows; ++q) {
    double val = 0.0;
    if (q == 0) val = s0;
    else if (q == 1) val = s1;
    else if (q < 2 + d) {
#pragma unroll
      for (int k = 0; k < DT; ++k)
        if (k == q - 2) val = g[k];
    } else if constexpr (MS) {
#pragma unroll
      for (int k = 0; k < DT; ++k)
        if (k == q - 2 - d) val = gm[k];
    }
    __syncthreads();
    red[rg * SM + col] = val;
    __syncthreads();
    if (tid < SM) a.kmred[(int64_t)q * a.mp + tid] = (red[tid] + red[SM + tid]) + (red[2 * SM + tid] + red[3 * SM + tid]);
  }
  if (a.wdiag && tid < SM) a.wdiag[tid] = Wt[tid * SLD + tid];
