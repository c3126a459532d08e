  constexpr int DP = DT * 16, LDP = DP + 4;
  __shared__ double zs[PG_CP * LDP];
  __shared__ double zn[PG_CP];
  __shared__ double ts[PG_CP];
  __shared__ double sh[DP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  if (tid < DP) sh[tid] = tid < a.d ? a.shift[tid] : 0.0;
  __syncthreads();
  const int row0 = blockIdx.x * PG_ROWS + wv * 16;
  const int prow = row0 + l15;  // the test point of this lane's elements of E
  const bool live_r = prow < a.rows;
  const int mc = (a.m + 15) & ~15;  // columns walked (<= mp)
  const ExpK ek = exp_consts();

  double pb[KS4], pn = 0.0;
#pragma unroll
  for (int s = 0; s < KS4; ++s) {
    const int k = 4 * s + lq;
    const double v = (live_r && k < a.d) ? a.pts[(int64_t)prow * a.d + k] - sh[k] : 0.0;
    pb[s] = v;
    pn += v * v;
  }
  pn += __shfl_xor(pn, 16);
  pn += __shfl_xor(pn, 32);
  pd4 accm[DT], accv[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) accm[t] = accv[t] = (pd4){0, 0, 0, 0};
  double rsm = 0.0, rsv = 0.0;
  const int pcol = 4 * (l15 & 3) + (l15 >> 2);  // A rows of the distance product: 0 4 8 12 1 5 ...

  // columns cb + 4 lq .. + 3 of row prow of G
  auto load_g = [&](int cb, double (&o)[4]) {
    if (VAR && live_r && cb < mc) {
      const pd2* q = reinterpret_cast<const pd2*>(a.G + (int64_t)prow * a.mp + cb + 4 * lq);
      const pd2 u = q[0], w = q[1];
      o[0] = u.x; o[1] = u.y; o[2] = w.x; o[3] = w.y;
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.0;
    }
  };
  double gv[4], gn[4];
  load_g(0, gv);
  for (int c0 = 0; c0 < mc; c0 += PG_CP) {
    __syncthreads();
    for (int idx = tid; idx < PG_CP * DP; idx += 256) {
      const int c = idx / DP, k = idx % DP, col = c0 + c;
      zs[c * LDP + k] = (col < a.m && k < a.d) ? a.Z[(int64_t)col * a.d + k] - sh[k] : 0.0;
    }
    if (tid < PG_CP) ts[tid] = c0 + tid < a.m ? a.tvec[c0 + tid] : 0.0;
    __syncthreads();
    {
      const int c = tid >> 2, q = tid & 3;
      double s2 = 0.0;
      for (int k = q; k < DP; k += 4) s2 += zs[c * LDP + k] * zs[c * LDP + k];
      s2 += __shfl_xor(s2, 1);
      s2 += __shfl_xor(s2, 2);
      if (q == 0) zn[c] = s2;
      __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < PG_CP / 16; ++j) {
      const int cb = c0 + 16 * j;
      if (cb >= mc) break;
      load_g(cb + 16, gn);  // (beyond the last column block: nothing)
      pd4 s4 = (pd4){0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < KS4; ++s) s4 = pmfma4(zs[(16 * j + pcol) * LDP + 4 * s + lq], pb[s], s4);
      double em[4], ev[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * j + 4 * lq + r;
        const double dist = fmax(pn + zn[c] - 2.0 * s4[r], 0.0);
        const double kv = (live_r && c0 + c < a.m) ? exp_fast(a.log_sf2 + a.inv_ell2_05 * dist, ek) : 0.0;
        em[r] = kv * ts[c];
        ev[r] = kv * gv[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        rsm += em[r];
        if constexpr (VAR) rsv += ev[r];
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          const double zv = zs[(16 * j + 4 * lq + r) * LDP + 16 * t + l15];
          accm[t] = pmfma4(em[r], zv, accm[t]);
          if constexpr (VAR) accv[t] = pmfma4(ev[r], zv, accv[t]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) gv[r] = gn[r];
    }
  }
  rsm += __shfl_xor(rsm, 16);
  rsm += __shfl_xor(rsm, 32);  // every lane: rowsum(E_mean) of test point l15 = its mean
  rsv += __shfl_xor(rsv, 16);
  rsv += __shfl_xor(rsv, 32);
  if (lq == 0 && live_r) {
    if (a.means) a.means[prow] = rsm;
    if (VAR && a.vars) a.vars[prow] = (a.sf2 - rsv) + a.add;
  }
  const double inv_ell2 = -2.0 * a.inv_ell2_05;
  if constexpr (ACQ || MV) {
    // the criterion of test point l15 from its mean and variance (all four lanes of a point alike); without the variance
    // part it is the bound with kappa = 0
    AcqPoint c;
    double* cvalues;
    if constexpr (MV) {
      // max-value entropy search (mv_math.h): lane lq of the point's four takes the extremes lq, lq + 4, ..., and the partial
      // sums are joined as rsm and rsv were -- a fixed order
      const double pvar = (a.sf2 - rsv) + a.add;
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
      if constexpr (VAR) {
        c = acq_point(q.kind, q.s, q.best, q.xi, q.kappa, q.var_floor, rsm, (a.sf2 - rsv) + a.add);
      } else {
        c.a = q.s * rsm;
        c.cmu = q.s;
        c.cv = 0.0;
      }
      cvalues = q.values;
    }
    if (lq == 0 && live_r && cvalues) cvalues[prow] = c.a;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = row0 + lq + 4 * r;
      const double rm = __shfl(rsm, lq + 4 * r), rv = __shfl(rsv, lq + 4 * r);
      const double cm = __shfl(c.cmu, lq + 4 * r), cv = __shfl(c.cv, lq + 4 * r);
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int dim = 16 * t + l15;
        if (orow < a.rows && dim < a.d && a.dmeans) {
          const double pc = a.pts[(int64_t)orow * a.d + dim] - sh[dim];
          const double dm = -inv_ell2 * (pc * rm - accm[t][r]);  // the entries the plain kernel stores
          double g = cm * dm;
          if constexpr (VAR) g += cv * (2.0 * inv_ell2 * (pc * rv - accv[t][r]));
          a.dmeans[(int64_t)orow * a.ldg + dim] = g;
        }
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = row0 + lq + 4 * r;
      const double rm = __shfl(rsm, lq + 4 * r), rv = __shfl(rsv, lq + 4 * r);
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int dim = 16 * t + l15;
        if (orow < a.rows && dim < a.d) {
          const double pc = a.pts[(int64_t)orow * a.d + dim] - sh[dim];
          if (a.dmeans) a.dmeans[(int64_t)orow * a.ldg + dim] = -inv_ell2 * (pc * rm - accm[t][r]);
          if (VAR && a.dvars) a.dvars[(int64_t)orow * a.ldg + dim] = 2.0 * inv_ell2 * (pc * rv - accv[t][r]);
        }
      }
    }
  }
