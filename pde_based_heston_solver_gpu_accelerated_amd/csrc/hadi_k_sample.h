// hadi_k_sample.h -- sampled ladder (hadi_sample_ladder and its launchers, include/hadi.h): the state of the v-row of V_0 evaluated
// at arbitrary spots on snapshot steps of a sweep, on the device.  hadi_sample_locate_kernel turns every (instance, sample) into a
// tap record once per call, before the sweep; hadi_sample_kernel applies the records behind a snapshot step of the streaming loop,
// hadi_sample_lds (hadi_k_small.h) inside the whole-loop LDS kernels.
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// One sample: four packed offsets row * rowp + hadi_pos(L, i) inside the instance's state, the Lagrange weights of the four
// s-nodes and the scale.  A node hit is the node's offset four times with the weights 1, 0, 0, 0: the chain below then returns the
// node's bits (0 * u + u = u for every finite u, signed zeros included).  off[0] < 0: the sample is off the grid or its stencil
// is degenerate -- the value is NaN and the sample's flag word says which.
struct HadiTap {
    int off[4];
    double w[4];
    double scale;
};
#define HADI_SAMPLE_OFF_GRID 1    // flag word: NaN spot, or a spot outside [s_0, s_m1] beyond the node tolerance
#define HADI_SAMPLE_DEGENERATE 2  // flag word: non-finite weights (a stencil with a zero interval, or m1 < 3)

// The value of a sample: at(off) reads the state at a packed offset.  One multiplication, three FMAs, one multiplication by the scale.
template <class F>
HADI_DEV HADI_FORCEINLINE double hadi_tap_value(const HadiTap &t, F &&at) {
    if (t.off[0] < 0) return nan("");
    const double u0 = at(t.off[0]), u1 = at(t.off[1]), u2 = at(t.off[2]), u3 = at(t.off[3]);
    return fma(t.w[3], u3, fma(t.w[2], u2, fma(t.w[1], u1, t.w[0] * u0))) * t.scale;
}

// One thread per (instance, sample).  vec_s / vec_v are the sweep's own device grids (a Jacobian's rebuilt per-group v-grids: the v0
// column samples its own row).  Row j0 by hadi_locate_kernel's rule: first v-node within 1e-10 of V_0 (V0_i[inst]), row 0 if none.
// With x the spot and s_0 < .. < s_m1 the instance's s-nodes:
//   node hit    the first i with |s_i - x| < 1e-10: a single tap
//   off grid    x NaN, x < s_0 or x > s_m1 (no node hit): flag HADI_SAMPLE_OFF_GRID
//   interior    i = the largest index with s_i < x, stencil i0 .. i0 + 3 with i0 = min(max(i - 1, 0), m1 - 3);
//               w_a = prod_{b != a} (x - s_{i0+b}) / prod_{b != a} (s_{i0+a} - s_{i0+b}), both products over increasing b, one division
//   degenerate  a non-finite weight: flag HADI_SAMPLE_DEGENERATE
// spots / scales: [n_inst][n_samp] (scales may be null = 1).  This is the one place where the comparisons and divisions happen.
__global__ void __launch_bounds__(256) hadi_sample_locate_kernel(HadiLayout L, int n_inst, int n_samp, const double *__restrict__ vec_s,
                                                                 const double *__restrict__ vec_v, const double *__restrict__ V0_i,
                                                                 double V_0, const double *__restrict__ spots,
                                                                 const double *__restrict__ scales, HadiTap *__restrict__ taps,
                                                                 int *__restrict__ flags) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n_inst * n_samp) return;
    const int inst = (int)(e / n_samp), m1 = L.m1;
    const double *s = vec_s + (size_t)inst * (m1 + 1);
    const double *v = vec_v + (size_t)inst * (L.m2 + 1);
    const double v0 = V0_i ? V0_i[inst] : V_0;
    const double x = spots[e];
    int j0 = 0;
    for (int j = 0; j <= L.m2; j++)
        if (fabs(v[j] - v0) < 1e-10) { j0 = j; break; }
    HadiTap t;
    t.scale = scales ? scales[e] : 1.0;
    int hit = -1, below = -1;  // the first node within the tolerance; the largest index with s_i < x
    for (int i = 0; i <= m1; i++) {
        if (hit < 0 && fabs(s[i] - x) < 1e-10) hit = i;
        if (s[i] < x) below = i;
    }
    int flag = 0;
    if (hit >= 0) {
        for (int a = 0; a < 4; a++) {
            t.off[a] = j0 * L.rowp + hadi_pos(L, hit);
            t.w[a] = a == 0 ? 1.0 : 0.0;
        }
    } else if (!(x >= s[0]) || !(x <= s[m1])) {  // (NaN fails both comparisons)
        flag = HADI_SAMPLE_OFF_GRID;
    } else if (m1 < 3) {
        flag = HADI_SAMPLE_DEGENERATE;
    } else {
        int i0 = below - 1;
        if (i0 < 0) i0 = 0;
        if (i0 > m1 - 3) i0 = m1 - 3;
        for (int a = 0; a < 4; a++) {
            double num = 1.0, den = 1.0;
            for (int b = 0; b < 4; b++)
                if (b != a) {
                    num *= x - s[i0 + b];
                    den *= s[i0 + a] - s[i0 + b];
                }
            t.w[a] = num / den;
            t.off[a] = j0 * L.rowp + hadi_pos(L, i0 + a);
            if (!(fabs(t.w[a]) <= 1.7976931348623157e308)) flag = HADI_SAMPLE_DEGENERATE;  // (inf or NaN)
        }
    }
    if (flag)
        for (int a = 0; a < 4; a++) { t.off[a] = -1; t.w[a] = 0.0; }
    taps[e] = t;
    flags[e] = flag;
}

// Streaming path of a sample call, in hadi_snap_kernel's place: snapshot q of every sample of every instance of a sub-batch, after
// the last pass of step snap_steps[q].  U, taps and out are the sub-batch's own (already offset); out[(inst * n_snap + q) * n_samp + s].
// Four gathered loads from the packed state and one store per thread.
__global__ void __launch_bounds__(256) hadi_sample_kernel(HadiLayout L, int n_inst, const double *__restrict__ U,
                                                          const HadiTap *__restrict__ taps, double *__restrict__ out, int n_snap,
                                                          int n_samp, int q) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n_inst * n_samp) return;
    const size_t inst = e / n_samp;
    const int s = (int)(e - inst * n_samp);
    const double *__restrict__ Ui = U + inst * L.inst_stride;
    const HadiTap t = taps[e];
    out[(inst * n_snap + q) * n_samp + s] = hadi_tap_value(t, [&](int off) { return Ui[off]; });
}
