// emu_small_jump_stage.cpp -- TEST-ONLY.  hadi_small_jump_stage<W> (csrc/hadi_k_small.h) ALONE under the wave emulator, on an LDS
// image laid out as hadi_small_body lays it out, and hadi_jump_step -- one launch of hadi_jump_kernel -- on the same packed rows,
// matrix and weight, so that the two routes' sub-steps can be set side by side bit for bit.  emu_jump_substep.cpp is included
// whole (and honours EMU_JUMP_SUBSTEP_ALONE, for tests/cpp/jump_substep_san.cpp).  Never shipped.
#include "emu_jump_substep.cpp"

// The image, in doubles, exactly the plan's smem_small_eu bytes (the block kernel's European LDS map):
//   [2 halo rows][U: nrows rows][2 halo rows][Y: nrows rows][coefficients 4 * 64 B][row table nrows * HADI_RCL][column table nrows * HADI_PBW]
// o8[8] (or NULL): B, rowp, nrows, doubles of the image, offset of U's row 0, offset of Y's row 0, offset of the first word behind
// Y's last row, hadi_jump_nib.  Returns the doubles of the image, or 0: the block kernel does not admit the shape.
extern "C" long long emu_small_jump_stage_layout(int m1, int m2, long long *o8) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, 1, 8 * 256, &pl, g_tune, 8) || pl.row_seq || pl.col_seq || !(pl.smem_small_eu > 0)) return 0;
    const HadiLayout &L = pl.L;
    const long long size = (long long)(pl.smem_small_eu / sizeof(double)), u0 = 2ll * L.rowp, y0 = (long long)(L.nrows + 4) * L.rowp;
    if (o8) {
        const long long v[8] = {L.B, L.rowp, L.nrows, size, u0, y0, y0 + (long long)L.nrows * L.rowp, hadi_jump_nib(L)};
        std::copy(v, v + 8, o8);
    }
    return size;
}

#ifndef EMU_JUMP_SUBSTEP_ALONE
// The route function's answer for a sampled Bates ladder of n instances with "jump_small" = 1 on a 256-CU part (canonical theta,
// r_d != r_f, two snapshots, ten samples): its description in desc; returns HadiRoute::kind, or -1 (refused).
extern "C" int emu_small_jump_route(int n, int m1, int m2, char *desc, int cap) {
    HadiRouteIn ri;
    ri.cu_count = 256; ri.n = n; ri.m1 = m1; ri.m2 = m2; ri.variant = HADI_EU; ri.scheme = HADI_SCHEME_DOUGLAS; ri.prec = 0;
    ri.theta = 0.8; ri.rates_equal = false; ri.debug = 0; ri.profiling = false; ri.n_snap = 2; ri.dividends = false;
    ri.uniform_steps = true; ri.team_failed = false; ri.jumps = true; ri.n_samp = 10;
    if (hadi_tuning_set(ri.t, *hadi_tuning_key("jump_small"), 1)) return -1;
    const HadiRoute r = hadi_route(ri);
    if (r.status) return -1;
    std::snprintf(desc, cap, "%s", hadi_describe_route(r, ri, false, HADI_TEAM_NOT_RUN).c_str());
    return (int)r.kind;
}
#endif

// field [(m2 + 1)(m1 + 1)], natural order: what the column pass left in U's node slots and the kernel copied to Y's.  The image in
// front of the stage: Y's node slots hold the field; U's node slots hold `stale` except column i = 0, which holds the field (row 0 of
// G is zero, so the stage rewrites that slot with the bits it finds in Y); EVERY other word -- the pad slots of U and Y, slots of
// nodes beyond m1, the four halo rows, the tables behind Y's last row -- holds `poison`.  W: 4 or 8 wavefronts.
// kind [image]: 0 a node slot of U, 1 a node slot of Y, 2 a pad slot of U or Y, 3 a halo row, 4 behind Y.
// img_in / img_out [image]: in front of and behind the stage.  step_in / step_out [nrows * rowp]: the packed rows hadi_jump_kernel was
// given (U's rows of the image with the field in every node slot) and left.  G_out [m1 + 1][m1 + 1]: the matrix, natural order.
// Returns 0, 1 (not admitted), 3 (bad W).
extern "C" int emu_small_jump_stage(int W, int m1, int m2, const double *vec_s, double mu, double sigma, const double *field, double a,
                                    double stale, double poison, double *img_in, double *img_out, unsigned char *kind, double *step_in,
                                    double *step_out, double *G_out) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, 1, 8 * 256, &pl, g_tune, 8) || pl.row_seq || pl.col_seq || !(pl.smem_small_eu > 0)) return 1;
    if (W != 4 && W != 8) return 3;
    const HadiLayout &L = pl.L;
    const int rowp = L.rowp, nrows = L.nrows;
    const size_t size = pl.smem_small_eu / sizeof(double), u0 = (size_t)2 * rowp, y0 = (size_t)(nrows + 4) * rowp, behind = y0 + (size_t)nrows * rowp;
    std::vector<double> img(size, poison);  // (sized as the LDS allocation is: a read or write past it is past this vector)
    for (size_t e = 0; e < size; e++) kind[e] = e >= behind ? 4 : 3;
    for (int j = 0; j < nrows; j++)
        for (int s = 0; s < rowp; s++) {
            const int i = hadi_slot_to_i(L, s);
            const bool node = i >= 0 && i <= m1;
            const size_t eu = u0 + (size_t)j * rowp + s, ey = y0 + (size_t)j * rowp + s;
            kind[eu] = node ? 0 : 2;
            kind[ey] = node ? 1 : 2;
            if (node) {
                const double f = field[(size_t)j * (m1 + 1) + i];
                img[ey] = f;
                img[eu] = i == 0 ? f : stale;
            }
        }
    std::copy(img.begin(), img.end(), img_in);
    const size_t gd = hadi_jump_matrix_doubles(L), ne = (size_t)(m1 + 1) * (m1 + 1);
    std::vector<double> G(gd, 0.0);
    const double musig[2] = {mu, sigma};
    emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_kernel(L, 1, vec_s, musig, G.data()); });
    emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_unpack_kernel(L, G.data(), G_out); });
    // ---- the stage, as hadi_small_body calls it: one block of W wavefronts, between two barriers ------------------------------
    double *Ul = img.data() + u0;
    const double *Yl = img.data() + y0;
    emu::launch(1, 64 * W, [&]() {
        const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
        __syncthreads();
        if (W == 4) hadi_small_jump_stage<4>(L, Yl, Ul, G.data(), a, wave, lane);
        else hadi_small_jump_stage<8>(L, Yl, Ul, G.data(), a, wave, lane);
        __syncthreads();
    });
    std::copy(img.begin(), img.end(), img_out);
    // ---- hadi_jump_step on the same rows: the packed state of one instance, U_temp = U, one launch of hadi_jump_kernel --------
    std::vector<double> dU((size_t)L.inst_stride, poison), dUT;
    for (int j = 0; j < nrows; j++)
        for (int s = 0; s < rowp; s++) {
            const int i = hadi_slot_to_i(L, s);
            if (i >= 0 && i <= m1) dU[(size_t)j * rowp + s] = field[(size_t)j * (m1 + 1) + i];
        }
    std::copy(dU.begin(), dU.begin() + (size_t)nrows * rowp, step_in);
    dUT = dU;
    HadiInstPar ipar{};
    ipar.N = 1;
    emu::launch(hadi_jump_grid(L, 1, 1), HADI_JUMP_THREADS, [&]() {
        hadi_jump_kernel(L, 1, 1, 0, 1, dUT.data(), dU.data(), G.data(), 0ll, &a, &ipar, 1);
    }, hadi_jump_smem(L));
    std::copy(dU.begin(), dU.begin() + (size_t)nrows * rowp, step_out);
    return 0;
}
