// Body shared by small_pass2_kernel and small_pass2_batch_kernel (small.hip includes it into both): `a` is the lane's argument struct.
  extern __shared__ __attribute__((aligned(16))) double small_lds[];
  double* const Ui = small_lds;          // [SM][SLD]  U^-1
  double* const Ri = Ui + SM * SLD;      // [SM][SLD]  R~^-1
  double* const Vt = Ri + SM * SLD;      // [SRB][SLD] V of the block
  double* const Qt = Vt + SRB * SLD;     // [SRB][SLD] Q', then X~, then X, each in place
  double* const xs = Qt + SRB * SLD;     // [SRB][DT]
  double* const isr = xs + SRB * DT;     // [SRB] per-row values of the block
  double* const vr = isr + SRB;
  double* const wr = vr + SRB;
  double* const esr = wr + SRB;
  double* const q2s = esr + SRB;
  double* const qbs = q2s + SRB;
  double* const bv = qbs + SRB;          // [SM] b
  double* const tt = bv + SM;            // [SM] t~
  double* const red = tt + SM;           // [4][SM] scratch of the final column reductions
  double* const iscL = red + 4 * SM;     // MS: [SM][DT] 1 / ms_kc
  double* const es2L = iscL + SM * DT;   // MS: [SRB][DT] sum_c E_rc / ms_kc of the block's rows
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const ExpK ek = exp_consts();
  const int d = a.d, D = a.D;
  load_corner(a.uinv, a.mp, Ui, tid);
  load_corner(a.rinv, a.mp, Ri, tid);
  if (tid < SM) {
    bv[tid] = a.bvec[tid];
    tt[tid] = a.ttil[tid];
  }
  if constexpr (MS) {
    for (int idx = tid; idx < SM * DT; idx += 256) {
      const int c = idx / DT, k = idx % DT;
      iscL[idx] = (k < d && c < a.m) ? 1.0 / a.cp.ms[(int64_t)c * d + k] : 0.0;
    }
  }
  const int col = lane, rg = wv;
  const bool live_c = col < a.m;
  // moments of E against the original inputs (`Proj derivative): per-thread sums for D <= 16; above that one more MFMA
  // product per block, X_big^T E, with the inputs staged where V was (WIDE)
  constexpr bool WIDE = DBT > 16 || MS;
  constexpr int NGB = WIDE ? 1 : DBT;
  double z[DT], gx[DT], gb[NGB];
  double isc[MS ? DT : 1], gxx[MS ? DT : 1], lsum = 0.0;
#pragma unroll
  for (int k = 0; k < DT; ++k) {
    z[k] = (k < d && live_c) ? a.Z[(int64_t)col * d + k] : 0.0;
    gx[k] = 0.0;
    if constexpr (MS) {
      const double scale = (k < d && live_c) ? a.cp.ms[(int64_t)col * d + k] : 1.0;
      isc[k] = 1.0 / scale;
      lsum += log(scale);
      gxx[k] = 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < NGB; ++k) gb[k] = 0.0;
  sd4 accGB[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) accGB[ct] = sd4{0.0, 0.0, 0.0, 0.0};
  sd4 accG[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) accG[ct] = sd4{0.0, 0.0, 0.0, 0.0};
  double cs = 0.0, sE = 0.0, sED = 0.0;
  double p_v = 0.0, p_is = 0.0, p_res = 0.0, p_v1 = 0.0;
  // `Proj second term: thread t accumulates outputs t, t + 256, ... of the D x d matrix
  constexpr int NPJ = (DBT * DT + 255) / 256;
  double pj[NPJ];
  int pj_big[NPJ], pj_small[NPJ];
#pragma unroll
  for (int j = 0; j < NPJ; ++j) {
    const int o = min(tid + 256 * j, max(D * d - 1, 0));
    pj[j] = 0.0;
    pj_big[j] = d > 0 ? o / d : 0;
    pj_small[j] = d > 0 ? o % d : 0;
  }
  const int nblk = a.rows_p / SRB;
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
    const int r0 = b * SRB;
    __syncthreads();
    for (int idx = tid; idx < SRB * DT; idx += 256) {
      const int r = idx / DT, k = idx % DT;
      xs[idx] = (k < d && r0 + r < a.rows) ? a.pts[(int64_t)(r0 + r) * d + k] : 0.0;
    }
    load_corner(a.V + (int64_t)r0 * a.mp, a.mp, Vt, tid);
    double kreg[KR ? 16 : 1];  // this thread's K entries of the block (column, 16 rows): requested now, used in the E phase
    if constexpr (KR) {
#pragma unroll
      for (int i = 0; i < 16; ++i) kreg[i] = a.Kin[(int64_t)(r0 + rg * 16 + i) * SM + col];
    }
    if (tid < SRB) isr[tid] = a.is[r0 + tid];
    const bool rowlive = tid < SRB && r0 + tid < a.rows;  // the row phase below: one thread per row
    const double rreg = rowlive ? a.r[r0 + tid] : 0.0;
    const double yreg = (rowlive && a.y) ? a.y[r0 + tid] : 0.0;
    __syncthreads();
    sd4 acc[4];
    rows_times<false, MS ? 4 : 8>(Vt, Ri, wv, l15, lq, acc);  // Q' = V R~^-1
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s2 = 0.0, sb = 0.0;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        s2 += acc[ct][r] * acc[ct][r];
        sb += acc[ct][r] * bv[16 * ct + l15];
      }
      s2 = sum16(s2);
      sb = sum16(sb);
      const int row = 16 * wv + lq + 4 * r;
      if (l15 == 0) {
        q2s[row] = s2;
        qbs[row] = sb;
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) Qt[row * SLD + 16 * ct + l15] = acc[ct][r];
    }
    __syncthreads();
    if (tid < SRB) {  // q_diag, w, v (as pass2_rows_kernel)
      const int row = r0 + tid;
      double w = 0.0, v = 0.0, es = 0.0;
      if (row < a.rows) {
        const double is = isr[tid], rr = rreg;
        const double qd = is * q2s[tid], sb = qbs[tid];
        const double y = yreg;
        const double res = a.y ? (y - sb) : 0.0;
        w = is * res;
        const double v1 = a.variational ? is * (2.0 - is * rr - qd) : is * (1.0 - qd);
        v = v1 - w * w;
        es = qd - v * (a.cp.sf2 - rr) - w * sb;
        p_v += v;
        p_is += is;
        p_res += w * res;
        p_v1 += v1;
      }
      a.w[row] = w;
      a.v[row] = v;
      if (a.es) a.es[row] = es;
      wr[tid] = w;
      vr[tid] = v;
      esr[tid] = es;
    }
    __syncthreads();
    rows_times<true, MS ? 4 : 8>(Qt, Ri, wv, l15, lq, acc);  // Q' R~^-T
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + lq + 4 * r;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int c = 16 * ct + l15;  // X~ = diag(is) Q' R~^-T - diag(v) V - w t~^T
        Qt[row * SLD + c] = isr[row] * acc[ct][r] - vr[row] * Vt[row * SLD + c] - wr[row] * tt[c];
      }
    }
    rows_times<true, MS ? 4 : 8>(Qt, Ui, wv, l15, lq, acc);  // X = X~ U^-T
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + lq + 4 * r;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        Qt[row * SLD + 16 * ct + l15] = acc[ct][r];
        if (a.X) a.X[(int64_t)(r0 + row) * a.mp + 16 * ct + l15] = acc[ct][r];
      }
    }
    gram_update(Vt, vr, wv, l15, lq, accG);  // G~ part = V^T diag(v) V
    __syncthreads();
    if constexpr (WIDE) {  // V is done with: its tile now holds the block's original inputs, zero-padded to 64 columns
      constexpr int DW = 64;
      for (int idx = tid; idx < SRB * DW; idx += 256) {
        const int r = idx / DW, k = idx % DW;
        Vt[r * SLD + k] = (k < D && r0 + r < a.rows) ? a.big[(int64_t)(r0 + r) * D + k] : 0.0;
      }
    }
    if constexpr (KR) {  // V is done with: its tile takes the block's K (rows of this wavefront)
      static_assert(!(KR && (DBT > 16 || MS)), "the staged-inputs variants need the tile themselves");
#pragma unroll
      for (int i = 0; i < 16; ++i) Vt[(rg * 16 + i) * SLD + col] = kreg[i];
    }
    // E = X .* K of the block: column sums, moments against the points (and the original inputs), sum E, sum E |x - z|^2
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int r = rg * 16 + i;
      double dist = MS ? lsum : 0.0;
#pragma unroll
      for (int k = 0; k < DT; ++k) {
        const double diff = xs[r * DT + k] - z[k];
        if constexpr (MS) dist += diff * diff * isc[k];
        else dist = dist + diff * diff;
      }
      [[maybe_unused]] const bool live = live_c && r0 + r < a.rows;
      double e;
      if constexpr (KR) e = Qt[r * SLD + col] * Vt[r * SLD + col];  // (K is zero on padded rows and columns)
      else e = live ? Qt[r * SLD + col] * exp_fast(a.cp.log_sf2 + a.cp.inv_ell2_05 * dist, ek) : 0.0;
#pragma unroll
      for (int k = 0; k < DT; ++k) {
        gx[k] += xs[r * DT + k] * e;
        if constexpr (MS) gxx[k] += xs[r * DT + k] * xs[r * DT + k] * e;
      }
      if constexpr (WIDE) {
        Qt[r * SLD + col] = e;  // (rows of this wavefront)
      } else if (D > 0 && r0 + r < a.rows) {
        const double* xb = a.big + (int64_t)(r0 + r) * D;
#pragma unroll
        for (int k = 0; k < NGB; ++k)
          if (k < D) gb[k] += xb[k] * e;
      }
      cs += e;
      sE += e;
      sED += e * dist;
    }
    if constexpr (WIDE) {
      __syncthreads();  // the staged inputs and E are complete
      if constexpr (MS) {  // es2[row][k] = sum_c E_rc / ms_kc: four threads per row, sixteen columns each
        const int row = tid >> 2, part = tid & 3;
        double sum[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) sum[k] = 0.0;
#pragma unroll 2
        for (int c = 16 * part; c < 16 * part + 16; ++c) {
          const double e = Qt[row * SLD + c];
#pragma unroll
          for (int k = 0; k < DT; ++k) sum[k] += e * iscL[c * DT + k];
        }
#pragma unroll
        for (int k = 0; k < DT; ++k) {
          double t = sum[k];
          t += __shfl_xor(t, 1);
          t += __shfl_xor(t, 2);
          if (part == 0) es2L[row * DT + k] = t;
        }
      }
      // accGB[ct] += (X_big^T E) tile (wv, ct): input dimensions 16 wv .. 16 wv + 15 against columns 16 ct ..
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double af[8], bf[8][4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 4 * (8 * h + j) + lq;
          af[j] = Vt[k * SLD + 16 * wv + l15];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) bf[j][ct] = Qt[k * SLD + 16 * ct + l15];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) accGB[ct] = mfma_f64(af[j], bf[j][ct], accGB[ct]);
      }
    }
    if (D > 0) {  // second term of the `Proj derivative: sum_r x_big,r p_small,r rowsum(E)_r  (MS: E / ms_small per column)
      if constexpr (MS) __syncthreads();
      const int nr = min(SRB, a.rows - r0);
      for (int r = 0; r < nr; ++r) {
#pragma unroll
        for (int j = 0; j < NPJ; ++j) {
          const double xb = WIDE ? Vt[r * SLD + pj_big[j]] : a.big[(int64_t)(r0 + r) * D + pj_big[j]];
          const double wgt = MS ? es2L[r * DT + pj_small[j]] : esr[r];
          pj[j] += xb * xs[r * DT + pj_small[j]] * wgt;
        }
      }
    }
  }
  constexpr int MSR = MS ? 1 : 0;
  const int ncq = 1 + d + D + MSR * d;  // rows of the column block
  double* part = a.part + (int64_t)blockIdx.x * p2len(d, D, MSR);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(16 * wv + lq + 4 * r) * SM + 16 * ct + l15] = accG[ct][r];
  double* pcol = part + SM * SM;
  // per-column accumulators: the four row groups of a column are combined in order
  if constexpr (WIDE) {  // these sums are complete (the MFMA product ran over all 64 rows of every block)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * wv + lq + 4 * r;
        if (k < D) pcol[(1 + d + k) * SM + 16 * ct + l15] = accGB[ct][r];
      }
  }
  for (int q = 0; q < ncq; ++q) {
    if (WIDE && q > d && q <= d + D) continue;  // (written above)
    double val = cs;
    if (q >= 1 && q <= d) {
#pragma unroll
      for (int k = 0; k < DT; ++k)
        if (k == q - 1) val = gx[k];
    } else if (q > d + D) {
      if constexpr (MS) {
#pragma unroll
        for (int k = 0; k < DT; ++k)
          if (k == q - 1 - d - D) val = gxx[k];
      }
    } else if (q > d) {
#pragma unroll
      for (int k = 0; k < NGB; ++k)
        if (k == q - 1 - d) val = gb[k];
    }
    __syncthreads();
    red[rg * SM + col] = val;
    __syncthreads();
    if (tid < SM) pcol[q * SM + tid] = (red[tid] + red[SM + tid]) + (red[2 * SM + tid] + red[3 * SM + tid]);
  }
  double* pproj = pcol + ncq * SM;
#pragma unroll
  for (int j = 0; j < NPJ; ++j)
    if (tid + 256 * j < D * d) pproj[tid + 256 * j] = pj[j];
  double* ptail = pproj + D * d;
  sE = sum64(sE);
  sED = sum64(sED);
  __syncthreads();
  if (lane == 0) {
    red[wv] = sE;
    red[4 + wv] = sED;
  }
  __syncthreads();
  if (wv == 0) {
    p_v = sum64(p_v);
    p_is = sum64(p_is);
    p_res = sum64(p_res);
    p_v1 = sum64(p_v1);
    if (lane == 0) {
      ptail[0] = p_v;
      ptail[1] = p_is;
      ptail[2] = p_res;
      ptail[3] = p_v1;
      ptail[4] = (red[0] + red[1]) + (red[2] + red[3]);
      ptail[5] = (red[4] + red[5]) + (red[6] + red[7]);
      ptail[6] = 0.0;
      ptail[7] = 0.0;
    }
  }
