  extern __shared__ __attribute__((aligned(16))) double pg_lds[];
  double* const Ui = pg_lds;            // [SM][SLD]
  double* const Ri = Ui + SM * SLD;     // [SM][SLD]
  double* const Kt = Ri + SM * SLD;     // [SRB][SLD] K
  double* const Wk = Kt + SRB * SLD;    // [SRB][SLD] V, Q, H, then E_var
  double* const zs = Wk + SRB * SLD;    // [SM][LDZ] Z - s (dimensions >= d zero)
  double* const xs = zs + SM * LDZ;     // [SRB][DT] test points
  double* const tv = xs + SRB * DT;     // [SM] mean coefficients
  double* const sh = tv + SM;           // [16] s
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const ExpK ek = exp_consts();
  const bool var = a.want_var != 0;
  if (var) {
    load_corner(a.uinv, a.mp, Ui, tid);
    load_corner(a.rinv, a.mp, Ri, tid);
  }
  if (tid < SM) tv[tid] = tid < a.m ? a.tvec[tid] : 0.0;
  if (tid >= 64 && tid < 80) sh[tid - 64] = tid - 64 < a.d ? a.shift[tid - 64] : 0.0;
  const int col = lane;
  const bool live_c = col < a.m;
  double z[DT];
#pragma unroll
  for (int k = 0; k < DT; ++k) z[k] = (k < a.d && live_c) ? a.Z[(int64_t)col * a.d + k] : 0.0;
  const int r0 = blockIdx.x * SRB;
  for (int idx = tid; idx < SRB * DT; idx += 256) {
    const int r = idx / DT, k = idx % DT;
    xs[idx] = (k < a.d && r0 + r < a.rows) ? a.pts[(int64_t)(r0 + r) * a.d + k] : 0.0;
    if constexpr (REFINE)  // the starts, clipped into the box
      if (k < a.d) xs[idx] = refine_clip(xs[idx], rf.lower[k], rf.upper[k]);
  }
  __syncthreads();
  for (int idx = tid; idx < SM * 16; idx += 256) {
    const int c = idx >> 4, k = idx & 15;
    zs[c * LDZ + k] = (c < a.m && k < a.d) ? a.Z[(int64_t)c * a.d + k] - sh[k] : 0.0;
  }
  // REFINE: what follows is one evaluation at the points in xs, inside the loop of the rule (rf_step, small_pg.h); the trip
  // count is the same for the whole workgroup
  [[maybe_unused]] RefineRows rr;
  [[maybe_unused]] bool rf_first = true, rf_more = false;
  if constexpr (REFINE) {
    const bool comp = l15 < a.d;
    rr.lo = comp ? rf.lower[l15] : 0.0;
    rr.hi = comp ? rf.upper[l15] : 0.0;
    rr.w = comp ? rr.hi - rr.lo : INFINITY;
    rr.sc = (comp && rf.scale) ? rf.scale[l15] : 1.0;
  }
  do {
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int r = wv * 16 + i;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k) {
      const double diff = xs[r * DT + k] - z[k];
      acc = acc + diff * diff;
    }
    Kt[r * SLD + col] = (r0 + r < a.rows && live_c) ? exp_fast(a.cp.log_sf2 + a.cp.inv_ell2_05 * acc, ek) : 0.0;
  }
  __syncthreads();
  // mean part: E_mean = K .* (1 t^T) formed as the A operand
  pd4 am = pd4{0.0, 0.0, 0.0, 0.0}, av = pd4{0.0, 0.0, 0.0, 0.0};
  double rsm = 0.0, rsv = 0.0;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int c = 4 * kk + lq;
    const double e = Kt[(16 * wv + l15) * SLD + c] * tv[c];
    rsm += e;
    am = pmfma4(e, zs[c * LDZ + l15], am);
  }
  if (var) {
    pd4 accv[4], acc[4];
    rows_times<false>(Kt, Ui, wv, l15, lq, accv);  // V = K U^-1
    store_rows(Wk, accv, wv, l15, lq);
    rows_times<false>(Wk, Ri, wv, l15, lq, acc);   // Q = V R~^-1
    store_rows(Wk, acc, wv, l15, lq);
    rows_times<true>(Wk, Ri, wv, l15, lq, acc);    // Q R~^-T
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = accv[ct] - acc[ct];  // H = V - Q R~^-T
    store_rows(Wk, acc, wv, l15, lq);
    rows_times<true>(Wk, Ui, wv, l15, lq, acc);    // G = H U^-T
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int o = (16 * wv + lq + 4 * r) * SLD + 16 * ct + l15;
        Wk[o] = Kt[o] * acc[ct][r];  // E_var = K .* G
      }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int c = 4 * kk + lq;
      const double e = Wk[(16 * wv + l15) * SLD + c];
      rsv += e;
      av = pmfma4(e, zs[c * LDZ + l15], av);
    }
  }
  rsm += __shfl_xor(rsm, 16);
  rsm += __shfl_xor(rsm, 32);  // every lane: the row sum of test point 16 wv + l15
  rsv += __shfl_xor(rsv, 16);
  rsv += __shfl_xor(rsv, 32);
  const int prow = r0 + 16 * wv + l15;
  if (lq == 0 && prow < a.rows) {
    if (a.means) a.means[prow] = rsm;
    if (var && a.vars) a.vars[prow] = (a.cp.sf2 - rsv) + a.add;
  }
  const double inv_ell2 = -2.0 * a.cp.inv_ell2_05;
  if constexpr (ACQ || MV) {
    // the criterion of test point 16 wv + l15 (all four lanes of a point alike); without the variance part it is the bound
    // with kappa = 0
    AcqPoint c;
    [[maybe_unused]] double* cvalues;
    if constexpr (MV) {
      // max-value entropy search (mv_math.h; the launch has seen to want_var): lane lq of the point's four takes the
      // extremes lq, lq + 4, ..., and the partial sums are joined as rsm and rsv were -- a fixed order
      const double pvar = (a.cp.sf2 - rsv) + a.add;
      const bool clamped = !(pvar >= mv.var_floor);
      const double v = clamped ? mv.var_floor : pvar, sigma = sqrt(v);
      MvSums t = mv_accumulate(mv.extremes, mv.n, lq, 4, mv.s, rsm, sigma);
      t.psi += __shfl_xor(t.psi, 16);
      t.psi += __shfl_xor(t.psi, 32);
      t.dpsi += __shfl_xor(t.dpsi, 16);
      t.dpsi += __shfl_xor(t.dpsi, 32);
      t.gdpsi += __shfl_xor(t.gdpsi, 16);
      t.gdpsi += __shfl_xor(t.gdpsi, 32);
      c = mv_finish(t, mv.n, mv.s, sigma, v, clamped);
      cvalues = mv.values;
    } else {
      if (var) {
        c = acq_point(q.kind, q.s, q.best, q.xi, q.kappa, q.var_floor, rsm, (a.cp.sf2 - rsv) + a.add);
      } else {
        c.a = q.s * rsm;
        c.cmu = q.s;
        c.cv = 0.0;
      }
      cvalues = q.values;
    }
    if constexpr (!REFINE)
      if (lq == 0 && prow < a.rows && cvalues) cvalues[prow] = c.a;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = 16 * wv + lq + 4 * r, orow = r0 + lrow;
      const double rm = __shfl(rsm, lq + 4 * r), rv = __shfl(rsv, lq + 4 * r);
      const double cm = __shfl(c.cmu, lq + 4 * r), cv = __shfl(c.cv, lq + 4 * r);
      if constexpr (REFINE) {
        rr.ay[r] = __shfl(c.a, lq + 4 * r);
        rr.gy[r] = 0.0;
      }
      if (orow < a.rows && l15 < a.d && (REFINE || a.dmeans)) {
        const double pc = xs[lrow * DT + l15] - sh[l15];
        const double dm = -inv_ell2 * (pc * rm - am[r]);  // the entries the plain kernel stores
        double g = cm * dm;
        if (var) g += cv * (2.0 * inv_ell2 * (pc * rv - av[r]));
        if constexpr (REFINE) rr.gy[r] = g;
        else a.dmeans[(int64_t)orow * a.ldg + l15] = g;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = 16 * wv + lq + 4 * r, orow = r0 + lrow;
      const double rm = __shfl(rsm, lq + 4 * r), rv = __shfl(rsv, lq + 4 * r);
      if (orow < a.rows && l15 < a.d) {
        const double pc = xs[lrow * DT + l15] - sh[l15];
        if (a.dmeans) a.dmeans[(int64_t)orow * a.ldg + l15] = -inv_ell2 * (pc * rm - am[r]);
        if (var && a.dvars) a.dvars[(int64_t)orow * a.ldg + l15] = 2.0 * inv_ell2 * (pc * rv - av[r]);
      }
    }
  }
  if constexpr (REFINE) {
    rf_more = __syncthreads_or(rf_step<DT>(a, rf, rr, xs, r0, wv, lq, l15, rf_first) ? 1 : 0) != 0;
    rf_first = false;
  }
  } while (REFINE && rf_more);
  if constexpr (REFINE) rf_store(a, rf, rr, r0, wv, lq, l15);
