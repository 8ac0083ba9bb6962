// hadi_k_lds_row_body.h -- the forward row sweep of the Douglas step of hadi_small_seq_kernel and hadi_small_seq2_kernel and its back
// substitution: lane <-> v-row, i = 1 .. m1 (same formulas as hadi_row_step).  NO include guard: the text is included into both
// kernels, inside `if (rowrun) { ... }`, so that both compile the very same statements -- their results are bit-identical, and the
// bits are those of the statements as they stand (as a function, or as a body shared through a template, the same expressions reach
// the backend with the operands of their two-product sums in another order, and hipcc fuses another product: DESIGN.md section 5,
// "Small-grid kernels on shared pieces").  The scheme is stated at the head of hadi_k_small.h's sequential kernels.
// Names the including kernel provides: the lane's row-table entry (v, wm, wz, wp, a2l2, a2l1, a2m, a2u1, a2u2, b1val, b1col, b1_at0),
// the instance's constants (dt, thdt, qd, half_rd, inv0, ip.hr0), this step's e_nm1, e_n, b1l, the pointers urow, yrow, crow, b2p,
// coefl, the wave shifts col5(own, m2v, m1v, p1v, p2v), and m1.
        // column i = 0 (A0 and A1 rows are zero there; only A2 and the boundary act)
        const double c00 = urow[0];
        double c0m2, c0m1, c0p1, c0p2;
        col5(c00, c0m2, c0m1, c0p1, c0p2);
        // first interior column, raw: rows j-2 .. j+2
        double r_0 = urow[1], r_m2, r_m1, r_p1, r_p2;
        col5(r_0, r_m2, r_m1, r_p1, r_p2);
        double yout_c0, x0;
        {
            const double a2c0 = a2l2 * c0m2 + a2l1 * c0m1 + a2m * c00 + a2u1 * c0p1 + a2u2 * c0p2;
            const double b1c0 = b1_at0 ? b1val : 0.0;
            const double b2c0 = b2p[0];
            const double a1c0 = -ip.hr0 * c00;  // A1 row 0: empty for the call (hr0 = 0), the reaction term for the put
            double y0c0 = c00 + dt * (a2c0 + a1c0 + (b1c0 + b2c0) * e_nm1);
            y0c0 = y0c0 + thdt * (b1c0 * e_n - (a1c0 + b1c0 * e_nm1));
            const double c2c0 = thdt * (b2c0 * e_n - (a2c0 + b2c0 * e_nm1));
            x0 = y0c0 * inv0;  // A1 row 0 is decoupled: the identity for the call (hes_a1_kernels.hpp:56-61)
            yout_c0 = x0 + c2c0;
        }
        hadi_wave_rendezvous();  // (emulator: everyone has read column 0 and 1 before c' overwrites column 0)
        double u_prev = c00, u_cur = r_0;
        double t_prev = wm * c0m1 + wz * c00 + wp * c0p1;
        double t_cur = wm * r_m1 + wz * r_0 + wp * r_p1;
        double a2u_cur = fma(a2u2, r_p2, fma(a2l2, r_m2, a2l1 * r_m1 + a2m * r_0 + a2u1 * r_p1));
        double b2c = b2p[1];
        double corr_cur = thdt * (b2c * e_n - (a2u_cur + b2c * e_nm1));
        // raw values of column 2 (column m1 + 1 is the zero spare)
        r_0 = urow[2];
        col5(r_0, r_m2, r_m1, r_p1, r_p2);
        // x_0 is known and moves to the right-hand side of node 1: with ys_0 = x_0 and c'_0 = 0 the general step does exactly
        // that (pivot im - il 0, right-hand side y - il x_0)
        double cp_prev = 0.0, ys_prev = x0;
        // One node of the sweep.  On entry r_* hold the raw column i + 1; `cB`, `cD` are node i's coefficients, `b2n` the b2
        // entry of node i + 1.  The caller refills r_* with column i + 2 afterwards.
        auto node = [&](int i, const double2 cB, const double2 cD, const double b2n) {
            const double u_next = r_0;
            const double t_next = wm * r_m1 + wz * r_0 + wp * r_p1;
            const double a2u_next = fma(a2u2, r_p2, fma(a2l2, r_m2, a2l1 * r_m1 + a2m * r_0 + a2u1 * r_p1));
            const double lo = fma(v, cD.x, qd * cB.x);
            const double up = fma(v, cD.y, qd * cB.y);
            const double mn = -((lo + up) + half_rd);
            const double A1U = lo * u_prev + mn * u_cur + up * u_next;
            const double A0U = cB.x * t_prev - (cB.x + cB.y) * t_cur + cB.y * t_next;
            // Y0 = U + dt (A0U + A1U + A2U + b e_{n-1}) + theta dt (b1 e_n - (A1U + b1 e_{n-1})), device_solver.hpp:236-250
            double S = A0U + A1U + a2u_cur;
            S += b2c * e_nm1;
            double y = fma(dt, S, u_cur);
            y = fma(-thdt, A1U, y);
            y += (i == b1col) ? b1l : 0.0;
            const double il = -thdt * lo;
            const double im = 1.0 - thdt * mn;
            const double iu = -thdt * up;
            const double inv = hadi_rcp(fma(-il, cp_prev, im));
            const double cp = iu * inv;
            const double ys = fma(-il, ys_prev, y) * inv;
            const double corr_next = thdt * (b2n * e_n - (a2u_next + b2n * e_nm1));
            yrow[i] = ys + corr_cur + cp * corr_next;  // g_i  (c'_{m1} = 0: the row ends there)
            crow[i - 1] = cp;
            u_prev = u_cur; u_cur = u_next;
            t_prev = t_cur; t_cur = t_next;
            a2u_cur = a2u_next; corr_cur = corr_next; b2c = b2n;
            cp_prev = cp; ys_prev = ys;
        };
        // Rounds of FOUR nodes: the own-row values of the columns i + 2 .. i + 5, the four nodes' coefficients and b2 entries
        // are all read first -- 16 independent LDS reads behind ONE wait -- then the four dependent steps run without touching
        // the LDS return path.  (Round 2 read five rows' values per node and waited for each node's coefficient and b2 reads:
        // ~900 LDS instructions per time step, and at the six wavefronts per CU that the 26 KB of an instance allow, the CU's
        // one LDS pipe was the busiest unit.)  Column indices reach i + 5 <= m1 + 2: the two zero spare columns of the pitch.
        int i = 1;
        for (; i + 3 <= m1; i += 4) {
            double Rm2[4], Rm1[4], R0[4], Rp1[4], Rp2[4], b2q[4];
            double2 cBq[4], cDq[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                R0[q] = urow[i + 2 + q];
                cBq[q] = *reinterpret_cast<const double2 *>(coefl + 4 * (i + q));
                cDq[q] = *reinterpret_cast<const double2 *>(coefl + 4 * (i + q) + 2);
                b2q[q] = b2p[i + 1 + q];  // (entry m1 + 1 is zero)
            }
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");  // (the reads stay in front of the four steps' stores)
#endif
            hadi_wave_rendezvous();  // (emulator: every lane has read its columns before anybody's c' lands in them)
#pragma unroll
            for (int q = 0; q < 4; q++) col5(R0[q], Rm2[q], Rm1[q], Rp1[q], Rp2[q]);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                node(i + q, cBq[q], cDq[q], b2q[q]);
                r_m2 = Rm2[q]; r_m1 = Rm1[q]; r_0 = R0[q]; r_p1 = Rp1[q]; r_p2 = Rp2[q];
                hadi_wave_rendezvous();  // (emulator: the lanes walk in lock step on the GPU)
            }
        }
        for (; i <= m1; i++) {  // the last m1 mod 4 nodes, one at a time
            const double n_0 = urow[i + 2];  // (column <= m1 + 2: a zero column)
            double n_m2, n_m1, n_p1, n_p2;
            col5(n_0, n_m2, n_m1, n_p1, n_p2);
            const double2 cB = *reinterpret_cast<const double2 *>(coefl + 4 * i);      // Bm, Bp
            const double2 cD = *reinterpret_cast<const double2 *>(coefl + 4 * i + 2);  // Dm, Dp
            const double b2n = b2p[i + 1];
            hadi_wave_rendezvous();
            node(i, cB, cD, b2n);
            r_m2 = n_m2; r_m1 = n_m1; r_0 = n_0; r_p1 = n_p1; r_p2 = n_p2;
            hadi_wave_rendezvous();  // (emulator: the lanes walk in lock step on the GPU)
        }
        hadi_lds_back_subst(yrow, crow, m1, yout_c0);  // (idle lanes walk their dummy row)
