// ocs_scan_body.inc -- the body of k_backward_scan and of k_backward_scan_tiled (ocs_scan_kernel.hpp).  A FRAGMENT, not a
// header: no include guard, included from inside the two function definitions, each of which defines the OCS_SC_ macros this
// text uses for whatever depends on the device layout (listed there) and removes them again.  `a` is the BwdArgsScan.
  constexpr int G = P::NS, NAUG = P::NAUG, TPW = 64 / G;
  static_assert(P::NC == 1 && P::NTC == 1 && P::ROW_SEPARABLE, "scan kernels: row-separable problems, one control");
  static_assert(L % G == 0 && W * L + 1 <= kScanPadFront && L + 1 <= 8, "chunk shape");
  typedef typename P::Stage Stage;
  // phase 3 from phase 1's affine step records where (dF/du)'v does not read y (registry problems); user problems
  // given as row functions (DFDU_READS_Y) form the stage states again
  constexpr bool AFF = !P::DFDU_READS_Y;
  __shared__ __attribute__((aligned(16))) double2 sm[2][W][64];      // chunk maps
  __shared__ double csm[2][64];                                      // lam at the bottom of a superblock
  __shared__ __attribute__((aligned(16))) double rcs[2][W][8 * kScanRec];   // records lo-1 .. lo+6 of a wave's chunk (1 KiB)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r = lane / TPW, tl = lane % TPW;   // trajectory fastest (see group_sum_sc)
  const size_t B = (size_t)a.batch;
  const int N = a.N;
  const int b0 = blockIdx.x * TPW + tl;
  const bool valid = b0 < a.batch;
  const int b = valid ? b0 : a.batch - 1;
  const uniform_ptr PS = as_uniform(a.ps);
  const typename P::RowPar rp = P::load_row(ParamSrc{PS, a.pb, a.pmask, B, b}, r);
  OCS_SC_PROLOGUE
  const double lamc = LT ? OCS_SC_LAMT(G) : 1.0;
  const size_t colB = (size_t)NAUG * OCS_SC_RX;
  double carry = LT ? OCS_SC_LAMT(r) : 0.0;   // lam(r, N+1)   :63-66
  if (OUT_LAM && wave == 0 && valid) {
    a.lam[OCS_SC_X0W (size_t)N * colB + (size_t)r * OCS_SC_RX + OCS_SC_LX] = carry;
    if (r == 0) a.lam[OCS_SC_X0W (size_t)N * colB + (size_t)G * OCS_SC_RX + OCS_SC_LX] = lamc;
  }
  const double pend_top = (OUT_DJDU && a.pend0 && r == 0) ? OCS_SC_PEND0 : 0.0;
  // per-lane parts of the addresses (bytes); the column parts are wave-uniform scalar offsets
  const unsigned col8 = (unsigned)(colB * 8), B8 = (unsigned)(OCS_SC_RU * 8);
  const unsigned vx = (unsigned)(((size_t)r * OCS_SC_RX + OCS_SC_LX) * 8);   // x loads (clamped lane: valid memory)
  const unsigned vu = (unsigned)(OCS_SC_LU * 8);                           // u loads
  const unsigned vl = valid ? vx : kOffDrop;                               // lam stores
  const unsigned vc = valid ? (unsigned)(((size_t)G * OCS_SC_RX + OCS_SC_LX) * 8) + (unsigned)r * col8 : kOffDrop;  // cost row of lam:
                                                                           // lane (trajectory, r) takes column lo + r (+ G k)
  // dJdu stores of step i = lo + q at scalar offset 2 q B: lane r = 0 the midpoint column 2i+1, r = 1 (or the
  // second store, G = 1) the node column 2i+2, r = 2 (G = 4) the chunk's lowest node column 2 lo with q = 0
  const bool is0 = r == 0, is1 = r == 1;
  const unsigned vd_mid = valid ? vu + B8 : kOffDrop, vd_node = valid ? vu + 2 * B8 : kOffDrop;
  const unsigned vd_bot = valid ? vu : kOffDrop;
  const unsigned vd_r = (G == 1) ? vd_mid : is0 ? vd_mid : is1 ? vd_node : kOffDrop;  // steps q > 0
  const unsigned vd_r0 = (G == 4 && r == 2) ? vd_bot : vd_r;                          // step q = 0

  struct Ld {
    double x0;            // x(r, lo): the checkpoint of the chunk's first step, the only one read (see above)
    double u[2 * L + 1];  // u(2 lo + k)
    double xb, ub0, ub1;  // DFDU_READS_Y only: x(r, lo-1), u(2 lo - 2), u(2 lo - 1) (stage state 4 of the step below)
  };
  // The loads of a chunk in L parts (part q: the records with q = 0, x(lo+q), u(2 lo + 2q), u(2 lo + 2q + 1),
  // and u(2 lo + 2L) with the last part), so that they can be issued between the steps of the previous superblock's
  // arithmetic: sixteen waves issuing 14 loads each back to back fill the address queue and stall at issue.
  auto load_part = [&](int sb, Ld& d, int slot, int q) OCS_INLINE {
    const int lo = scan_chunk_lo<W, L>(N, sb, wave), lc = lo > 0 ? lo : 0;
    // the records first: older in the in-order queue than the loads the compiler waits for
    // (a dead chunk -- below step 0, possibly far below in a superblock past the horizon -- takes zero records
    //  from the front pad: identity maps)
    const int lr = lo >= 0 ? lo - 1 : -kScanPadFront;
    if (q == 0) dma16(a.RECS + (long long)lr * kScanRec + 2 * lane, &rcs[slot][wave][0]);
    const Buf bx = Buf::make(a.xck + OCS_SC_X0W (size_t)lc * colB), bu = Buf::make(a.u + OCS_SC_U0W (size_t)(2 * lc) * OCS_SC_RU);
    if (q == 0) d.x0 = bx.ld(vx, 0);
    d.u[2 * q] = bu.ld(vu, (unsigned)(2 * q) * B8);
    d.u[2 * q + 1] = bu.ld(vu, (unsigned)(2 * q + 1) * B8);
    if (q == L - 1) d.u[2 * L] = bu.ld(vu, (unsigned)(2 * L) * B8);
    if (P::DFDU_READS_Y && q == 0) {
      const int lb = lo > 0 ? lo - 1 : 0;   // (lo = 0: the values are multiplied by a zero record)
      const Buf bxb = Buf::make(a.xck + OCS_SC_X0W (size_t)lb * colB), bub = Buf::make(a.u + OCS_SC_U0W (size_t)(2 * lb) * OCS_SC_RU);
      d.xb = bxb.ld(vx, 0);
      d.ub0 = bub.ld(vu, 0);
      d.ub1 = bub.ld(vu, B8);
    }
  };
  auto load = [&](int sb, Ld& d, int slot) OCS_INLINE {
#pragma unroll
    for (int q = 0; q < L; ++q) load_part(sb, d, slot, q);
  };
  constexpr int NST = (OUT_LAM ? L + L / G : 0) + (OUT_DJDU ? (G == 1 ? 2 * L + 1 : (G == 2 ? L + 1 : L)) : 0);
  struct Rc { double h, hh, h6, h3, s4, s3, s1, tA, tM, tB; };
  auto rec_of = [&](const double* w, int q) OCS_INLINE {   // record of step lo + q (q = -1: the step below the chunk)
    const double2* p = reinterpret_cast<const double2*>(w + (q + 1) * kScanRec);
    const double2 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4], a5 = p[5];   // (unused fields cost nothing)
    return Rc{a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a4.x, a4.y, a5.x};
  };

  auto process = [&](int sb, const Ld& d, int slot, bool first, Ld& dn) OCS_INLINE {
    const int lo = scan_chunk_lo<W, L>(N, sb, wave);
    const bool live = lo >= 0, topc = lo + L == N;
    // the records have landed once everything up to this superblock's loads has (in-order vmcnt); younger: the
    // previous superblock's stores (the loads of the next superblock are issued inside phase 1, after this wait)
    if (first)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
    const double* rw = &rcs[slot][wave][0];
    // ---------------- phase 1: stage states and the chunk map ----------------
    // Steps in ascending order: only the checkpoint of the chunk's first step was read, the next one comes out
    // of the stage evaluations the step map needs anyway plus one more right-hand side (RK4Integrator.m:49-50 on this row)
    // -- 8 nS / L instead of 8 nS bytes of checkpoint traffic per (trajectory, step).  The chunk map is composed from the
    // bottom: lam_lo = A lam_(above the steps so far) + Bq.
    double xs[L];
    xs[0] = d.x0;
    double A = 1.0, Bq = 0.0;
    // AFF: what phase 3 needs of step i = lo + q, as affine functions of lam_{i+1}, kept instead of the stage states:
    // lam_i (al, be), the midpoint column p23 (mp, mq), the k1 half of node column 2i (c1 kp, kq_i) and the k4 half of
    // node column 2i+2 (c4 h6, fq_i), with c v + d = (dF/du)'v of a stage (g_row_dfdu_v, g_row_dfdu_0); c1 and c4 read
    // the record only and are applied in phase 3.  The constants of a node column are kept as one: nq[q] = fq_i +
    // kq_{i+1} (q < L-1), nq[L-1] = fq of the top step, nb = kq_lo + the constant of the k4 half of step lo-1.
    double al[L], be[L], mp[L], mq[L], kp[L], nq[L], nb = 0.0;
#pragma unroll
    for (int q = 0; q < L; ++q) {
      const Rc c = rec_of(rw, q);
      const double xi = xs[q], uA = d.u[2 * q], uM = d.u[2 * q + 1], uB = d.u[2 * q + 2];
      const double F1 = P::g_row_f(xi, uA, c.tA, rp);           // compute_states :39-46, this row
      const double Y2 = __builtin_fma(c.hh, F1, xi);
      const double F2 = P::g_row_f(Y2, uM, c.tM, rp);
      const double Y3 = __builtin_fma(c.hh, F2, xi);
      const double F3 = P::g_row_f(Y3, uM, c.tM, rp);
      const double Y4 = __builtin_fma(c.h, F3, xi);
      if (q + 1 < L) {
        const double F4 = P::g_row_f(Y4, uB, c.tB, rp);
        xs[q + 1] = __builtin_fma(c.h6, ((F1 + 2.0 * F2) + 2.0 * F3) + F4, xi);   // :50
      }
      const Stage s4 = P::template stage<LT>(c.s4, c.h6, c.tB, lamc), s3 = P::template stage<LT>(c.s3, c.h3, c.tM, lamc),
                  s1 = P::template stage<LT>(c.s1, c.h6, c.tA, lamc);
      // row of (dF/dy)'v = a v_r + b; (p, q): the quantity is p lam_{i+1} + q          :73-88
      double a4, b4, a3, b3, a2, b2, a1, b1;
      P::g_row_dfdx_pre(Y4, uB, s4, rp, a4, b4);
      const double g3p = a4 * c.h6, g3q = b4;                                   // k4 = (h6, 0)
      const double k3p = __builtin_fma(c.h, g3p, c.h3), k3q = c.h * g3q;
      P::g_row_dfdx_pre(Y3, uM, s3, rp, a3, b3);
      const double g2p = a3 * k3p, g2q = __builtin_fma(a3, k3q, b3);
      const double k2p = __builtin_fma(c.hh, g2p, c.h3), k2q = c.hh * g2q;
      P::g_row_dfdx_pre(Y2, uM, s3, rp, a2, b2);
      const double g1p = a2 * k2p, g1q = __builtin_fma(a2, k2q, b2);
      const double k1p = __builtin_fma(c.hh, g1p, c.h6), k1q = c.hh * g1q;
      P::g_row_dfdx_pre(xi, uA, s1, rp, a1, b1);
      const double g0p = a1 * k1p, g0q = __builtin_fma(a1, k1q, b1);
      const double alpha = (((1.0 + g1p) + g2p) + g3p) + g0p;
      const double beta = ((g1q + g2q) + g3q) + g0q;
      Bq = __builtin_fma(A, beta, Bq);
      A = A * alpha;
      if constexpr (AFF) {
        al[q] = alpha;
        be[q] = beta;
        if (OUT_DJDU) {   // (dF/du)'v = c v + d per stage; stages 2 and 3 share u and the stage values  :97-121
          const double c3 = P::g_row_dfdu_v(s3, rp), d3 = P::g_row_dfdu_0(uM, s3, rp), c1 = P::g_row_dfdu_v(s1, rp);
          mp[q] = c3 * k3p + c3 * k2p;
          mq[q] = __builtin_fma(c3, k3q, d3) + __builtin_fma(c3, k2q, d3);
          kp[q] = k1p;
          const double kq = __builtin_fma(c1, k1q, P::g_row_dfdu_0(uA, s1, rp));
          if (q == 0) {
            const Rc cb = rec_of(rw, -1);
            nb = kq + P::g_row_dfdu_0(uA, P::template stage<LT>(cb.s4, cb.h6, cb.tB, lamc), rp);
          } else {
            nq[q - 1] += kq;
          }
          nq[q] = P::g_row_dfdu_0(uB, s4, rp);
          // formed here, not sunk below the barrier (that would keep u, the stage values and the k pairs alive instead)
          asm volatile("" : "+v"(mp[q]), "+v"(mq[q]), "+v"(kp[q]));
          if (q == 0) asm volatile("" : "+v"(nb));
          if (q > 0) asm volatile("" : "+v"(nq[q - 1]));
          if (q == L - 1) asm volatile("" : "+v"(nq[q]));
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // one step at a time: the temporaries of interleaved steps cost occupancy
      load_part(sb + 1, dn, slot ^ 1, q);
      __builtin_amdgcn_sched_barrier(0);
    }
    sm[sb & 1][wave][lane] = double2{A, Bq};
    lds_barrier();
    // ---------------- phase 2: lam at the top of this chunk ----------------
    double lam = (sb == 0) ? carry : csm[(sb & 1) ^ 1][lane];
#pragma unroll
    for (int j0 = 0; j0 < W; j0 += 4) {
      if (j0 < wave) {   // wave-uniform
        double2 ab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ab[j] = sm[sb & 1][j0 + j][lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j0 + j < wave) {   // wave-uniform; the fence keeps it a branch (two selects per map otherwise)
            lam = __builtin_fma(ab[j].x, lam, ab[j].y);
            asm volatile("" : "+v"(lam));
          }
        }
      }
    }
    // ---------------- phase 3: the recursion inside the chunk, lam and dJdu stores ----------------
    const int lc = live ? lo : 0, nrec = live ? kNumRec : 0;   // a dead chunk stores nothing
    const Buf bl = Buf::make(a.lam + OCS_SC_X0W (size_t)lc * colB, nrec), bd = Buf::make(a.dJdu + OCS_SC_U0W (size_t)(2 * lc) * OCS_SC_RU, nrec);
    if (OUT_LAM) {
      // the constant cost row of lam for the L columns of the chunk
#pragma unroll
      for (int q0 = 0; q0 < L; q0 += G) bl.st(lamc, vc, (unsigned)q0 * col8);
    }
    double pend = topc ? pend_top : 0.0;   // this row's B'k1 share of the node above
    double lt2 = 0.0;                        // (AFF) lam_{i+2}
#pragma unroll
    for (int q = L - 1; q >= 0; --q) {
      // lam_i and this row's shares of column 2i+1 (p23), column 2i+2 (pn) and, q = 0, column 2 lo (pb)   :73-121
      double p23 = 0.0, pn = 0.0, pb = 0.0;
      if constexpr (AFF) {
        const double lt = lam;                                   // lam_{i+1}
        lam = __builtin_fma(al[q], lt, be[q]);
        if (OUT_DJDU) {
          // c of the stage-4 half of step lo + j, times h6 (k4 = h6 lam), and of the stage-1 half
          auto c4h6 = [&](int j) OCS_INLINE {
            const Rc r = rec_of(rw, j);
            return P::g_row_dfdu_v(P::template stage<LT>(r.s4, r.h6, r.tB, lamc), rp) * r.h6;
          };
          auto c1 = [&](int j) OCS_INLINE {
            const Rc r = rec_of(rw, j);
            return P::g_row_dfdu_v(P::template stage<LT>(r.s1, r.h6, r.tA, lamc), rp);
          };
          p23 = __builtin_fma(mp[q], lt, mq[q]);
          pn = __builtin_fma(c4h6(q), lt, nq[q]);
          if (q == L - 1)
            pn = pend + pn;
          else
            pn = __builtin_fma(c1(q + 1) * kp[q + 1], lt2, pn);
          if (q == 0)   // column 2 lo: the k1 half of step lo, the k4 half of step lo-1 (k4 = h/6 lam_lo)
            pb = __builtin_fma(c4h6(-1), lam, __builtin_fma(c1(0) * kp[0], lt, nb));
          lt2 = lt;
        }
      } else {
        const Rc c = rec_of(rw, q);
        // the stage states again (held registers are worth more than these nine operations: 4 waves per SIMD)
        const double xi = xs[q], uA = d.u[2 * q], uM = d.u[2 * q + 1], uB = d.u[2 * q + 2];
        double f = P::g_row_f(xi, uA, c.tA, rp);
        const double Y2 = __builtin_fma(c.hh, f, xi);
        f = P::g_row_f(Y2, uM, c.tM, rp);
        const double Y3 = __builtin_fma(c.hh, f, xi);
        f = P::g_row_f(Y3, uM, c.tM, rp);
        const double Y4 = __builtin_fma(c.h, f, xi);
        const Stage s4 = P::template stage<LT>(c.s4, c.h6, c.tB, lamc), s3 = P::template stage<LT>(c.s3, c.h3, c.tM, lamc),
                    s1 = P::template stage<LT>(c.s1, c.h6, c.tA, lamc);
        const double h6l = c.h6 * lam, h3l = c.h3 * lam;
        const double k4 = h6l;                                     // :73
        const double g3 = P::g_row_dfdx(Y4, uB, k4, s4, rp);       // :74-75
        const double k3 = __builtin_fma(c.h, g3, h3l);             // :77
        const double g2 = P::g_row_dfdx(Y3, uM, k3, s3, rp);       // :78-79
        const double k2 = __builtin_fma(c.hh, g2, h3l);            // :81
        const double g1 = P::g_row_dfdx(Y2, uM, k2, s3, rp);       // :82-83
        const double k1 = __builtin_fma(c.hh, g1, h6l);            // :85
        const double g0 = P::g_row_dfdx(xi, uA, k1, s1, rp);       // :87-88
        lam = (((lam + g1) + g2) + g3) + g0;                       // :86-88
        if (OUT_DJDU) {                                            // compute_dJdu :97-121
          const double p4 = P::g_row_dfdu(Y4, uB, k4, s4, rp);
          p23 = P::g_row_dfdu(Y3, uM, k3, s3, rp) + P::g_row_dfdu(Y2, uM, k2, s3, rp);
          pn = pend + p4;
          pend = P::g_row_dfdu(xi, uA, k1, s1, rp);
          if (q == 0) {
            // column 2 lo = B'k1 of step lo + B'k4 of step lo-1 (k4 = h/6 lam_lo); column 0 has the k1 half only
            // :101-102.  Where (dF/du)'v reads y, stage state 4 of the step below is recomputed from three extra loads.
            const Rc cb = rec_of(rw, -1);
            const Stage sb4 = P::template stage<LT>(cb.s4, cb.h6, cb.tB, lamc);
            double Y4b = 0.0;
            if (P::DFDU_READS_Y) {
              double fb = P::g_row_f(d.xb, d.ub0, cb.tA, rp);
              const double Y2b = __builtin_fma(cb.hh, fb, d.xb);
              fb = P::g_row_f(Y2b, d.ub1, cb.tM, rp);
              const double Y3b = __builtin_fma(cb.hh, fb, d.xb);
              fb = P::g_row_f(Y3b, d.ub1, cb.tM, rp);
              Y4b = __builtin_fma(cb.h, fb, d.xb);
            }
            pb = pend + P::g_row_dfdu(Y4b, uA, cb.h6 * lam, sb4, rp);
          }
        }
      }
      if (OUT_LAM) bl.st(lam, vl, (unsigned)q * col8);
      if (OUT_DJDU) {
        // column 2i+1 (sum of p23 over the rows) and column 2i+2 (sum of pn; it belongs to the chunk of step i+1,
        // except column 2N): lanes of row 0 end up with the first, lanes of row 1 with the second
        double cmid, cnode;
        if (G == 1) {
          cmid = p23;
          cnode = pn;
        } else {
          cmid = cnode = pair_sum_sc<G>(p23, pn);
        }
        const unsigned so = (unsigned)(2 * q) * B8;
        const double cbot = (q == 0) ? group_sum_sc<G>(pb) : 0.0;
        if (G == 1) {
          bd.st(cmid, vd_mid, so);
          if (q == L - 1)
            bd.st(cnode, topc ? vd_node : kOffDrop, so);
          else
            bd.st(cnode, vd_node, so);
          if (q == 0) bd.st(cbot, vd_bot, so);
        } else {
          // (cmid = cnode here; above q = 0 the lanes of rows 2 and 3 store nothing)
          const double val = (q == 0 && !is0 && !is1) ? cbot : cmid;
          if (q == L - 1)
            bd.st(val, (topc | is0) ? vd_r : kOffDrop, so);
          else if (q == 0 && G == 4)
            bd.st(val, vd_r0, so);
          else
            bd.st(val, vd_r, so);
          if (q == 0 && G == 2) bd.st(cbot, is0 ? vd_bot : kOffDrop, so);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (wave == W - 1) csm[sb & 1][lane] = lam;   // lam at the bottom of the superblock (a dead chunk passes it through)
    carry = lam;
  };

  // Superblocks in pairs (two register sets, no register moves); a superblock past the horizon loads clamped
  // addresses and processes identity maps without a store, so the loop needs no conditions.
  const int nsb = (N + W * L - 1) / (W * L);
  Ld d0, d1;
  load(0, d0, 0);
  for (int sb = 0; sb < nsb; sb += 2) {
    process(sb, d0, 0, sb == 0, d1);
    process(sb + 1, d1, 1, false, d0);
  }
  if (a.lam0 && wave == W - 1 && valid) {   // the last wave's chunk ends at (or, dead, passes through) step 0
    a.lam0[(size_t)r * B + b] = carry;
    if (r == 0) a.lam0[(size_t)G * B + b] = lamc;
  }
