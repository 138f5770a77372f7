// The per-pixel loop of mandel_perturb_bla.hip, included TEXTUALLY into the body of each of its kernels (no include guard: it is a
// fragment, not a header).  In scope at the include: a (the kernel's arguments), gx, gy (the lane's column and row in the dc / u table)
// and valid (false: the lane runs no trip).  It leaves n (the count) and trips (the loop trips) behind.
// MC_BLA_ON_ESCAPE(zx, zy) is the includer's: empty, or the smooth instantiation's capture of the escaping z (mandel_smooth.h).
// Why not a __device__ function: the tile kernel's listing is the project's invariant, and the same loop inlined from a function comes
// out of the register allocator with the operands of one v_add3_u32 swapped and one v_mov_b32 moved.  Lexically inside the kernel it is
// unchanged.
    const double2* __restrict__ Z = a.t.orbit;
    const double* __restrict__ T = a.bla;
    const uint32_t L = a.t.L, M = a.t.max_iter;
    const uint64_t n0 = L >= 3u ? (uint64_t)L - 2u : 0u;   // level 0's entries
    const uint64_t s0 = level_sum(n0);
    const double dcx = a.t.table[valid ? gx : 0u], dcy = a.t.table[a.t.W + (valid ? gy : 0u)];
    double dx = 0.0, dy = 0.0;
    uint32_t m = 0u, i = valid ? 0u : M, n = M, trips = 0u;
    while (i < M) {
        trips++;
        // the step's orbit entries, issued before the probes (m <= L-1 here, so m + 1 <= L)
        const double2 zm = Z[m], z1 = Z[m + 1u];
        // kcap: the largest k the alignment ((m-1) divisible by 2^k), the orbit's end (m + 2^k <= L-1) and the iterations left
        // (i + 2^k <= M) allow; 0 = no level (m = 0, or fewer than two steps before Z_(L-1))
        uint32_t kcap = 0u;
        if (m >= 1u && L - 1u - m >= 2u) {
            const uint32_t ka = m == 1u ? 31u : (uint32_t)__builtin_ctz(m - 1u);
            const uint32_t kl = 31u - (uint32_t)__builtin_clz(L - 1u - m);
            const uint32_t ki = 31u - (uint32_t)__builtin_clz(M - i);
            kcap = ka < kl ? ka : kl;
            kcap = kcap < ki ? kcap : ki;
        }
        const double nd = fabs(dx) + fabs(dy);
        uint32_t k = 0u;
        double Ax = 0.0, Ay = 0.0, Bx = 0.0, By = 0.0;
        if (kcap >= 1u) {
            // probe(kk): is N1(d) < R_kk(m)?  On success the entry's (A, B) are kept
            auto probe = [&](uint32_t kk) -> bool {
                const uint64_t e = (s0 - level_sum(n0 >> kk)) + (uint64_t)((m - 1u) >> kk);
                const double* t = T + 5u * e;
                const double ax = t[0], ay = t[1], bx = t[2], by = t[3], r = t[4];
                if (!(nd < r)) return false;
                Ax = ax; Ay = ay; Bx = bx; By = by;
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
        if (k) {   // skip 2^k iterations: no escape test, no rebase test
            const double ndx = ((Ax * dx) - (Ay * dy)) + ((Bx * dcx) - (By * dcy));
            const double ndy = ((Ax * dy) + (Ay * dx)) + ((Bx * dcy) + (By * dcx));
            dx = ndx; dy = ndy;
            m = m + (1u << k);
            i = i + (1u << k);
        } else {   // PERTURB's iteration i, exactly
            const double ax = (zm.x + zm.x) + dx, ay = (zm.y + zm.y) + dy;
            const double ndx = ((ax * dx) - (ay * dy)) + dcx;
            const double ndy = ((ax * dy) + (ay * dx)) + dcy;
            m = m + 1u;
            const double zx = z1.x + ndx, zy = z1.y + ndy;
            const double r = (zx * zx) + (zy * zy);
            if (r > 2.0) { MC_BLA_ON_ESCAPE(zx, zy) n = i; break; }
            if (m == L || r < ((ndx * ndx) + (ndy * ndy))) { dx = zx; dy = zy; m = 0u; }   // rebase onto Z_0
            else { dx = ndx; dy = ndy; }
            i = i + 1u;
        }
    }
