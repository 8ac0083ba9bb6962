// jump_substep_san.cpp -- TEST-ONLY, stand-alone.  The emulated Bates sub-step (tests/emu/emu_jump_substep.cpp, included whole: the
// kernels of csrc/hadi_k_jumps.h compiled for the host) over every shape of tests/jump_cases.py, meant to be built with
// -fsanitize=address,undefined and run as a program (tests/test_cpp_jump_substep_san.py): every index the matrix kernel, the
// product and its staging compute -- operand order, K padding, tiles of U, the lists of hadi_jump_sel_kernel -- is checked against
// the bounds of plain std::vector buffers sized exactly as the library sizes its own.  Each launch is also held to the isolation
// rule in long double (jump_cases.substep_ratio), so a run that stays inside its buffers but multiplies wrongly fails as well.
// Likewise hadi_small_jump_stage<W>, the sub-step of the whole-loop kernel, on every shape of tests/bates_domain_cases.py (run_stage).
#define EMU_JUMP_SUBSTEP_ALONE 1
#include "../emu/emu_small_jump_stage.cpp"  // (includes emu_jump_substep.cpp whole)

#include <cinttypes>

static const int M1_EDGES[] = {2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024};
static const int M2_EDGES[] = {3, 14, 15, 16, 47, 48, 62, 63, 64, 127, 128, 527};
static const double LAWS[][2] = {{0.5, 1.0}, {-1.0, 0.5}, {0.0, 2.0}, {-0.10, 0.15}, {0.10, 0.30}, {-0.20, 0.25}, {-0.3, 0.4}, {0.2, 0.6}, {-0.5, 0.8}};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uniform01() {  // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (double)((g_rng * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

// A monotone s-grid on [0, 800 + 10 q], denser around 100: s_i = 100 + c sinh(xi), as the project's builder shapes its own.
static void make_grid(int m1, int q, double *s) {
    const double lo = std::asinh(-100.0 / 20.0), hi = std::asinh((700.0 + 10.0 * q) / 20.0);
    for (int i = 0; i <= m1; i++) s[i] = 100.0 + 20.0 * std::sinh(lo + (hi - lo) * i / m1);
    s[0] = 0.0;
}

struct Case { int kernel, m1, m2, n_src, n, o, cnt, width, shared, per, share; };

static int run_case(const Case &c) {
    const int m1p = c.m1 + 1, nrows = c.m2 + 1, n_mat = c.kernel ? HADI_JUMP_SETS * c.per : (c.shared ? 1 : c.n_src);
    const size_t m = (size_t)m1p * nrows;
    long long lay[10];
    const long long size = emu_jump_substep_layout(c.n, c.m1, c.m2, lay);
    if (size <= 0) { std::printf("FAIL no layout for %dx%d\n", c.m1, c.m2); return 1; }
    std::vector<double> grids((size_t)c.n_src * m1p), vs_mat((size_t)n_mat * m1p), musig(2 * (size_t)n_mat), U((size_t)c.n * m), avec(c.n);
    for (int q = 0; q < c.n_src; q++) make_grid(c.m1, c.shared || (c.kernel && c.per == 1) ? 0 : q, grids.data() + (size_t)q * m1p);
    for (int q = 0; q < n_mat; q++) {
        std::copy(grids.begin() + (size_t)(q % c.n_src) * m1p, grids.begin() + (size_t)(q % c.n_src + 1) * m1p, vs_mat.begin() + (size_t)q * m1p);
        musig[2 * q] = LAWS[q % 9][0];
        musig[2 * q + 1] = LAWS[q % 9][1];
    }
    for (int k = 0; k < c.n; k++) {
        avec[k] = (k & 1) ? 0.37 : 1.0;
        for (int j = 0; j < nrows; j++)
            for (int i = 0; i < m1p; i++) U[(size_t)k * m + (size_t)j * m1p + i] = (0.5 + uniform01()) * (1.0 + grids[(size_t)(k % c.n_src) * m1p + i]);
    }
    std::vector<double> P0((size_t)size), P1((size_t)size), Uo((size_t)c.n * m), G((size_t)n_mat * m1p * m1p);
    std::vector<unsigned char> pad((size_t)size);
    const int rc = emu_jump_substep(c.kernel, c.n, c.m1, c.m2, n_mat, vs_mat.data(), musig.data(), U.data(), avec.data(), nullptr, c.o, c.cnt,
                                    c.n_src, c.width, c.shared, c.per, c.share, std::nan(""), P0.data(), P1.data(), pad.data(), Uo.data(),
                                    G.data());
    if (rc) { std::printf("FAIL rc %d\n", rc); return 1; }
    int fails = 0;
    const size_t stride = (size_t)size / c.n;
    for (size_t e = 0; e < (size_t)size; e++) {
        const int k = (int)(e / stride);
        if ((pad[e] || k < c.o || k >= c.o + c.cnt) && std::memcmp(&P0[e], &P1[e], 8)) fails++;
    }
    if (fails) std::printf("FAIL %d elements outside the launch's nodes changed\n", fails);
    // the isolation rule, long double (64-bit significand on x86-64)
    const long double u = std::ldexp(1.0L, -53), K = (long double)lay[4] + 2, gam = K * u / (1 - K * u);
    long double worst = 0;
    for (int k = c.o; k < c.o + c.cnt; k++) {
        const int g = k / c.n_src, mat = c.kernel ? hadi_jump_set(g) * c.per + (c.per > 1 ? k % c.n_src : 0) : (c.shared ? 0 : k % c.n_src);
        const double *Gm = G.data() + (size_t)mat * m1p * m1p;
        for (int j = 0; j < nrows; j++) {
            const double *p = U.data() + (size_t)k * m + (size_t)j * m1p, *w = Uo.data() + (size_t)k * m + (size_t)j * m1p;
            for (int i = 0; i < m1p; i++) {
                long double r = 0, sa = 0;
                for (int l = 0; l < m1p; l++) {
                    r += (long double)p[l] * Gm[(size_t)i * m1p + l];
                    sa += std::fabs((long double)p[l] * Gm[(size_t)i * m1p + l]);
                }
                const long double err = std::fabs(((long double)w[i] - p[i]) - avec[k] * r);
                const long double bound = avec[k] * gam * sa + 2 * u * std::max(std::fabs((long double)w[i]), std::fabs((long double)p[i]));
                if (!(err <= bound)) fails++;
                if (bound > 0) worst = std::max(worst, err / bound);
            }
        }
    }
    std::printf("%s %4dx%-3d n %2d [%d, %d) width %d shared %d per %d share %d: worst %.3Lf of the bound%s\n", c.kernel ? "sel  " : "plain", c.m1,
                c.m2, c.n, c.o, c.o + c.cnt, c.width, c.shared, c.per, c.share, worst, fails ? "  FAIL" : "");
    return fails ? 1 : 0;
}

// hadi_small_jump_stage<W> alone (tests/emu/emu_small_jump_stage.cpp) on an image sized exactly as the block kernel's LDS allocation:
// a read or write of the stage past it is past a std::vector.  Nothing but U's nodes may change, and U's rows must be hadi_jump_step's
// bits on the same rows (whose product the cases above hold to the isolation rule).
static int run_stage(int m1, int m2, int W) {
    long long o8[8];
    const long long size = emu_small_jump_stage_layout(m1, m2, o8);
    if (size <= 0) { std::printf("FAIL no block-kernel layout for %dx%d\n", m1, m2); return 1; }
    const int m1p = m1 + 1, nrows = m2 + 1, rowp = (int)o8[1];
    std::vector<double> s(m1p), field((size_t)m1p * nrows), in((size_t)size), out((size_t)size), r0((size_t)nrows * rowp), r1((size_t)nrows * rowp),
        G((size_t)m1p * m1p);
    std::vector<unsigned char> kind((size_t)size);
    make_grid(m1, 0, s.data());
    for (int j = 0; j < nrows; j++)
        for (int i = 0; i < m1p; i++) field[(size_t)j * m1p + i] = (0.5 + uniform01()) * (1.0 + s[i]);
    const double a = (W == 4) ? 1.0 : 0.37;
    const int rc = emu_small_jump_stage(W, m1, m2, s.data(), LAWS[(m1 + W) % 3][0], LAWS[(m1 + W) % 3][1], field.data(), a, -12345.0, std::nan(""),
                                        in.data(), out.data(), kind.data(), r0.data(), r1.data(), G.data());
    if (rc) { std::printf("FAIL stage rc %d\n", rc); return 1; }
    int fails = 0, moved = 0;
    for (size_t e = 0; e < (size_t)size; e++) {
        if (kind[e] != 0 && std::memcmp(&in[e], &out[e], 8)) fails++;
        if (kind[e] == 0 && std::memcmp(&in[e], &out[e], 8)) moved++;
    }
    if (std::memcmp(out.data() + o8[4], r1.data(), sizeof(double) * nrows * rowp)) fails++;
    if (moved != nrows * m1) fails++;  // (every node but column i = 0)
    std::printf("stage %4dx%-3d W %d: %d nodes rewritten%s\n", m1, m2, W, moved, fails ? "  FAIL" : "");
    return fails ? 1 : 0;
}

int main() {
    int fails = 0;
    {   // the shapes of tests/bates_domain_cases.py; the largest m2 at 128 by the plan's own admission, walked up from 128x20
        const int rows[][2] = {{16, 11}, {63, 24}, {64, 31}, {64, 32}, {127, 16}, {128, 20}, {50, 32}, {100, 12}};
        int top = 20;
        while (emu_small_jump_stage_layout(128, top + 1, nullptr) > 0) top++;
        for (int W : {4, 8}) {
            for (auto &r : rows) fails += run_stage(r[0], r[1], W);
            fails += run_stage(128, top, W);
        }
    }
    for (int m1 : M1_EDGES) {
        const int big = m1 >= 512;
        fails += run_case(Case{0, m1, big ? 3 : 12, big ? 1 : 2, big ? 1 : 2, 0, big ? 1 : 2, 1, 0, 0, 0});
    }
    for (int m2 : M2_EDGES) fails += run_case(Case{0, 50, m2, 2, 2, 0, 2, 1, 0, 0, 0});
    for (int o : {0, 1, 2, 4})
        for (int ipg : {1, 3, 8}) fails += run_case(Case{0, 50, 12, 3, 18, o, 7, ipg, 0, 0, 0});
    fails += run_case(Case{0, 300, 12, 1, 7, 0, 7, 3, 1, 0, 0});
    const int ranges[][2] = {{0, 14}, {14, 13}, {4, 22}, {19, 8}};
    for (auto &r : ranges) {
        fails += run_case(Case{1, 50, 12, 3, 27, r[0], r[1], 1, 0, 3, 0});
        for (int cap : {1, 3, 7}) fails += run_case(Case{1, 50, 12, 3, 27, r[0], r[1], cap, 0, 3, 1});
    }
    fails += run_case(Case{1, 300, 12, 3, 27, 14, 13, 3, 0, 1, 0});
    fails += run_case(Case{1, 513, 3, 3, 27, 14, 13, 7, 0, 3, 1});
    std::printf(fails ? "FAILED (%d)\n" : "all sub-step shapes passed\n", fails);
    return fails ? 1 : 0;
}
