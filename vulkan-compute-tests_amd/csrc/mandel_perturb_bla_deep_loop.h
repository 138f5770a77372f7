// The per-pixel loop of mandel_perturb_bla_deep.hip, included TEXTUALLY into the body of each of its kernels (no include guard: it is a
// fragment, not a header).  In scope at the include: a (the kernel's arguments), gx, gy (the lane's column and row in the dc / u table)
// and valid (false: the lane runs no trip).  It leaves n (the count) and trips (the loop trips) behind.
// MC_BLA_ON_ESCAPE(zx, zy) is the includer's: empty, or the smooth instantiation's capture of the escaping z (mandel_smooth.h).
// Why not a __device__ function: the tile kernel's listing is the project's invariant, and the same loop inlined from a function comes
// out of the register allocator with the operands of one v_add3_u32 swapped and two v_ldexp_f64 pairs in another order.  Lexically
// inside the kernel it is unchanged.
    const double2* __restrict__ Z = a.t.orbit;
    const BlaDeepRec* __restrict__ T = a.bla;
    const uint32_t L = a.t.L, M = a.t.max_iter;
    const int32_t E = a.exp2;
    const uint64_t n0 = L >= 3u ? (uint64_t)L - 2u : 0u;   // level 0's entries
    const uint64_t s0 = level_sum(n0);
    const double ux = a.t.table[valid ? gx : 0u], uy = a.t.table[a.t.W + (valid ? gy : 0u)];
    double wx = 0.0, wy = 0.0, dx = 0.0, dy = 0.0;   // delta = w * 2^S;  d = ldexp(w, S)
    int32_t S = E;
    bool scaled = true;
    uint32_t m = 0u, i = valid ? 0u : M, n = M, trips = 0u;
    while (i < M) {
        trips++;
        // the step's orbit entries, issued before the probes (m <= L-1 here, so m + 1 <= L)
        const double2 zm = Z[m], z1 = Z[m + 1u];
        uint32_t kcap = 0u;
        if (m >= 1u && L - 1u - m >= 2u) {
            const uint32_t ka = m == 1u ? 31u : (uint32_t)__builtin_ctz(m - 1u);
            const uint32_t kl = 31u - (uint32_t)__builtin_clz(L - 1u - m);
            const uint32_t ki = 31u - (uint32_t)__builtin_clz(M - i);
            kcap = ka < kl ? ka : kl;
            kcap = kcap < ki ? kcap : ki;
        }
        const double nw = fabs(wx) + fabs(wy);
        uint32_t k = 0u;
        double Ax = 0.0, Ay = 0.0, Bx = 0.0, By = 0.0;
        int32_t eA = 0, eB = 0;
        if (kcap >= 1u) {
            // probe(kk): is N1(w) 2^S < R_kk(m)?  On success the entry's (A, B) are kept
            auto probe = [&](uint32_t kk) -> bool {
                const uint64_t e = (s0 - level_sum(n0 >> kk)) + (uint64_t)((m - 1u) >> kk);
                const BlaDeepRec t = T[e];
                if (!(ldexp2(nw, S - t.er) < t.r)) return false;
                Ax = t.ax; Ay = t.ay; Bx = t.bx; By = t.by; eA = t.ea; eB = t.eb;
                return true;
            };
            if (probe(1u)) {
                uint32_t lo = 1u, hi = kcap;   // level lo passes; the answer is in [lo, hi]
                if (hi > lo) {
                    if (probe(hi)) lo = hi;
                    else hi = hi - 1u;
                }
                while (lo < hi) {
                    const uint32_t mid = (lo + hi + 1u) >> 1;
                    if (probe(mid)) lo = mid;
                    else hi = mid - 1u;
                }
                k = lo;   // lo moves only on a passing probe, so (A, B) are level lo's entry
            }
        }
        if (k) {   // skip 2^k iterations: delta' = A delta + B u 2^E in floatexp; no escape test, no rebase test
            const double px = (Ax * wx) - (Ay * wy), py = (Ax * wy) + (Ay * wx);
            const double qx = (Bx * ux) - (By * uy), qy = (Bx * uy) + (By * ux);
            const double ap = fmax(fabs(px), fabs(py)), aq = fmax(fabs(qx), fabs(qy));
            const int32_t eP = eA + S, eQ = eB + E;
            double sx, sy;
            int32_t e;
            if (ap == 0.0) { sx = qx; sy = qy; e = eQ; }
            else if (aq == 0.0) { sx = px; sy = py; e = eP; }
            else {
                const int32_t kp = eP + frexp_exp(ap), kq = eQ + frexp_exp(aq);
                e = kp > kq ? kp : kq;
                sx = ldexp2(px, eP - e) + ldexp2(qx, eQ - e);
                sy = ldexp2(py, eP - e) + ldexp2(qy, eQ - e);
            }
            const double as = fmax(fabs(sx), fabs(sy));   // normalise: (sx, sy) 2^e with max part in [0.5, 1), or exactly 0
            if (as == 0.0) {
                wx = wy = dx = dy = 0.0;
                S = E;
                scaled = true;
            } else {
                const int32_t ks = frexp_exp(as);
                sx = ldexp2(sx, -ks); sy = ldexp2(sy, -ks);
                e = e + ks;
                dx = ldexp2(sx, e); dy = ldexp2(sy, e);
                if (fmax(fabs(dx), fabs(dy)) >= kT) { scaled = false; S = 0; wx = dx; wy = dy; }
                else { scaled = true; S = e; wx = sx; wy = sy; }
            }
            m = m + (1u << k);
            i = i + (1u << k);
        } else {   // §3.7's rescaled iteration i, exactly
            double nwx, nwy;
            int32_t nS = S;
            if (scaled && zm.x == 0.0 && zm.y == 0.0) {                     // Z_m = 0: a fresh exponent
                nS = max(S + S, E);
                const double px = pow2((S + S) - nS), pu = pow2(E - nS);
                nwx = (((wx * wx) - (wy * wy)) * px) + (ux * pu);
                nwy = (((wx * wy) + (wy * wx)) * px) + (uy * pu);
            } else {
                const double pu = pow2(E - S);
                const double ax = (zm.x + zm.x) + dx, ay = (zm.y + zm.y) + dy;
                nwx = ((ax * wx) - (ay * wy)) + (ux * pu);
                nwy = ((ax * wy) + (ay * wx)) + (uy * pu);
            }
            const double ndx = ldexp2(nwx, nS), ndy = ldexp2(nwy, nS);
            m = m + 1u;
            const double zx = z1.x + ndx, zy = z1.y + ndy;
            const double r = (zx * zx) + (zy * zy);
            if (r > 2.0) { MC_BLA_ON_ESCAPE(zx, zy) n = i; break; }
            if (m == L || r < ((ndx * ndx) + (ndy * ndy))) {                 // rebase: Z_0 = 0, delta = z
                m = 0u;
                dx = zx; dy = zy;
                const double am = fmax(fabs(zx), fabs(zy));
                if (am >= kT) { scaled = false; S = 0; wx = zx; wy = zy; }
                else {
                    scaled = true;
                    S = am == 0.0 ? E : frexp_exp(am);                       // exactly 0: restart as at the start
                    wx = ldexp2(zx, -S); wy = ldexp2(zy, -S);
                }
            } else {
                wx = nwx; wy = nwy; dx = ndx; dy = ndy; S = nS;
                if (scaled) {
                    if (fmax(fabs(ndx), fabs(ndy)) >= kT) { scaled = false; S = 0; wx = ndx; wy = ndy; }
                    else {
                        const double am = fmax(fabs(nwx), fabs(nwy));
                        if (am > kWinHi || am < kWinLo) {
                            const int32_t e = frexp_exp(am);
                            wx = ldexp2(nwx, -e); wy = ldexp2(nwy, -e);
                            S = nS + e;
                        }
                    }
                }
            }
            i = i + 1u;
        }
    }
