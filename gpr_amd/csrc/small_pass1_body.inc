// Body shared by small_pass1_kernel and small_pass1_batch_kernel (small.hip includes it into both): `a` is the lane's argument struct.
  extern __shared__ __attribute__((aligned(16))) double small_lds[];
  double* const Ui = small_lds;         // [SM][SLD]  U^-1
  double* const Kt = Ui + SM * SLD;     // [SRB][SLD] K of the block, then V in place
  double* const xs = Kt + SRB * SLD;    // [SRB][DT]
  double* const isr = xs + SRB * DT;    // [SRB] 1/s
  double* const yisr = isr + SRB;       // [SRB] y/s
  double* const rs = yisr + SRB;        // [SRB] rowsum(V.^2)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const ExpK ek = exp_consts();
  load_corner(a.uinv, a.mp, Ui, tid);
  const int col = lane, rg = wv;  // covariance / column-sum phases: thread = (column, group of 16 rows)
  const bool live_c = col < a.m;
  double z[DT], sc[MS ? DT : 1], lsc[MS ? DT : 1];
#pragma unroll
  for (int k = 0; k < DT; ++k) {
    z[k] = (k < a.d && live_c) ? a.Z[(int64_t)col * a.d + k] : 0.0;
    if constexpr (MS) {
      sc[k] = (k < a.d && live_c) ? a.cp.ms[(int64_t)col * a.d + k] : 1.0;
      lsc[k] = log(sc[k]);
    }
  }
  sd4 accB[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) accB[ct] = sd4{0.0, 0.0, 0.0, 0.0};
  double csum = 0.0, p_log = 0.0, p_y2 = 0.0, p_isr = 0.0;
  const int nblk = a.rows_p / SRB;
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
    const int r0 = b * SRB;
    __syncthreads();
    for (int idx = tid; idx < SRB * DT; idx += 256) {
      const int r = idx / DT, k = idx % DT;
      xs[idx] = (k < a.d && r0 + r < a.rows) ? a.pts[(int64_t)(r0 + r) * a.d + k] : 0.0;
    }
    const double yreg = (tid < SRB && a.y && r0 + tid < a.rows) ? a.y[r0 + tid] : 0.0;  // used by the row phase below
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int r = rg * 16 + i;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < DT; ++k) {  // (dimensions beyond d are zero on both sides, scale 1: they add exactly 0)
        const double diff = xs[r * DT + k] - z[k];
        if constexpr (MS) acc = (acc + diff * (diff / sc[k])) + lsc[k];
        else acc = acc + diff * diff;
      }
      const double kv = (r0 + r < a.rows && live_c) ? exp_fast(a.cp.log_sf2 + a.cp.inv_ell2_05 * acc, ek) : 0.0;
      Kt[r * SLD + col] = kv;
      if (a.Kout) a.Kout[(int64_t)(r0 + r) * SM + col] = kv;  // kept for pass 2 (E = X .* K without a second exp)
    }
    __syncthreads();
    sd4 acc[4];
    rows_times<false>(Kt, Ui, wv, l15, lq, acc);  // V = K U^-1
    double s2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s = 0.0;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) s += acc[ct][r] * acc[ct][r];
      s2[r] = sum16(s);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + lq + 4 * r;
      if (l15 == 0) rs[row] = s2[r];
      double* vrow = a.V + (int64_t)(r0 + row) * a.mp;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        Kt[row * SLD + 16 * ct + l15] = acc[ct][r];  // rows of this wavefront only: in place
        vrow[16 * ct + l15] = acc[ct][r];
        vrow[SM + 16 * ct + l15] = 0.0;  // columns 64..127 of the padded store
      }
    }
    __syncthreads();
    if (tid < SRB) {  // r, s = r + sigma2, 1/s, sum log s  (as pass1_rows_kernel)
      const int row = r0 + tid;
      double rr = 0.0, is = 0.0, yis = 0.0;
      if (row < a.rows) {
        rr = a.cp.sf2 - rs[tid];
        const double s = rr + a.sigma2;
        is = 1.0 / s;
        const double y = yreg;
        yis = is * y;
        p_log += log(s);
        p_y2 += is * y * y;
        p_isr += is * rr;
      }
      a.r[row] = rr;
      a.is[row] = is;
      a.yis[row] = yis;
      isr[tid] = is;
      yisr[tid] = yis;
    }
    __syncthreads();
    gram_update(Kt, isr, wv, l15, lq, accB);
    for (int i = 0; i < 16; ++i) {
      const int k = rg * 16 + i;
      csum += Kt[k * SLD + col] * yisr[k];
    }
  }
  double* part = a.part + (int64_t)blockIdx.x * P1LEN;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(16 * wv + lq + 4 * r) * SM + 16 * ct + l15] = accB[ct][r];
  __syncthreads();
  Kt[rg * SLD + col] = csum;
  __syncthreads();
  if (tid < SM) part[SM * SM + tid] = (Kt[tid] + Kt[SLD + tid]) + (Kt[2 * SLD + tid] + Kt[3 * SLD + tid]);
  if (wv == 0) {
    p_log = sum64(p_log);
    p_y2 = sum64(p_y2);
    p_isr = sum64(p_isr);
    if (lane == 0) {
      part[SM * SM + SM + 0] = p_log;
      part[SM * SM + SM + 1] = p_y2;
      part[SM * SM + SM + 2] = p_isr;
      part[SM * SM + SM + 3] = 0.0;
    }
  }
