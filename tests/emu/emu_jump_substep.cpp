// emu_jump_substep.cpp -- TEST-ONLY.  ONE launch of the Bates sub-step under the wave emulator, on a packed state the caller
// chooses: emu_jumps8.cpp (included whole) plus an entry point that packs a natural field as hadi_pack_kernel does, poisons
// every element of the packed state that is no node, builds the matrices (hadi_jump_matrix_kernel into a zeroed buffer) and makes
// the launch of hadi_jump_kernel or hadi_jump_sel_kernel that enqueue_sub_batch of hadi_api.hip makes for the sub-batch
// [o, o + cnt) of the batch: the pointers UT, U, avec and ipar moved to instance o, inst0 = o, and ipg / HadiJumpSel as
// jump_ipg / jump_sel set them (the caller passes their values).  Never shipped.
#ifdef EMU_JUMP_SUBSTEP_ALONE
// (tests/cpp/jump_substep_san.cpp: the kernels' headers alone -- none of the other drivers and not the table of instantiations,
// which a sanitizer build would instrument for minutes)
#define HADI_EMU 1
#include "hadi_kernels.h"
#include "hadi_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace emu {
thread_local emu_dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockState *t_block;
thread_local WaveState *t_wave;
thread_local int t_lane;
}  // namespace emu
static HadiTuning g_tune;
#else
#include "emu_jumps8.cpp"
#endif

// o10[10] (or NULL): rowp, nrows, nrows_pad, inst_stride, the padded K extent 4 hadi_jump_kg, hadi_jump_nib, B, G, HADI_JUMP_UP,
// HADI_JUMP_KC.  Returns the elements of the packed state of n_inst instances, or 0 (no streaming plan).
extern "C" long long emu_jump_substep_layout(int n_inst, int m1, int m2, long long *o10) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8) || pl.row_seq || pl.col_seq) return 0;
    const HadiLayout &L = pl.L;
    if (o10) {
        const long long v[10] = {L.rowp, L.nrows, L.nrows_pad, L.inst_stride, 4ll * hadi_jump_kg(L), hadi_jump_nib(L), L.B, L.G,
                                 HADI_JUMP_UP, HADI_JUMP_KC};
        std::copy(v, v + 10, o10);
    }
    return (long long)L.inst_stride * n_inst;
}

// kernel 0: hadi_jump_kernel -- instance k of the batch uses matrix k % n_src (shared: the one matrix, g_stride 0), `width`
// instances per block (ipg).  kernel 1: hadi_jump_sel_kernel -- the batch is 9 groups of n_src, HadiJumpSel{o, n_src, per, share,
// cap = width}.  n_mat matrices: matrix q on the grid vec_s [q][m1 + 1] with (musig[2 q], musig[2 q + 1]).
// U [n_inst][m]: the field in front of the sub-step (not modified).  avec [n_inst]: the weights a_k.  done [n_inst] (or NULL):
// 1 = the instance has finished (n > N_k).  poison: what every pad slot, slot beyond m1 and identity row of the packed state holds
// in front of the launch (NaN is the point: whatever the kernel reads of it shows).
// P_in, P_out [emu_jump_substep_layout]: the packed state in front of and behind the launch; is_pad, same size: 1 where the
// element is no node.  U_out [n_inst][m]: P_out unpacked.  G_out [n_mat][m1 + 1][m1 + 1]: the matrices, natural order
// (hadi_jump_matrix_unpack_kernel).
// Returns 0, 1 (no streaming plan), 3 (not admitted).
extern "C" int emu_jump_substep(int kernel, int n_inst, int m1, int m2, int n_mat, const double *vec_s, const double *musig,
                                const double *U, const double *avec, const int *done, int o, int cnt, int n_src, int width, int shared,
                                int per, int share, double poison, double *P_in, double *P_out, unsigned char *is_pad, double *U_out,
                                double *G_out) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8) || pl.row_seq || pl.col_seq) return 1;
    const HadiLayout &L = pl.L;
    if (o < 0 || cnt < 1 || o + cnt > n_inst || width < 1 || n_src < 1 || n_mat < 1) return 3;
    if (kernel == 0 ? n_mat != (shared ? 1 : n_src)
                    : (kernel != 1 || n_inst != HADI_JUMP_GROUPS * n_src || n_mat != HADI_JUMP_SETS * per || (per != 1 && per != n_src) ||
                       (share && per != n_src) || width > 8))
        return 3;
    const size_t st = (size_t)L.inst_stride * n_inst, gd = hadi_jump_matrix_doubles(L), ne = (size_t)(m1 + 1) * (m1 + 1);
    std::vector<double> dU(st), dUT, G((size_t)n_mat * gd, 0.0);
    std::vector<HadiInstPar> ipar(n_inst);
    for (int k = 0; k < n_inst; k++) ipar[k].N = (done && done[k]) ? 0 : 1;
    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U, dU.data()); });
    for (size_t e = 0; e < st; e++) {
        const size_t r = e % (size_t)L.inst_stride;
        const int i = hadi_slot_to_i(L, (int)(r % L.rowp));
        is_pad[e] = (i < 0 || i > L.m1 || (int)(r / L.rowp) >= L.nrows) ? 1 : 0;
        if (is_pad[e]) dU[e] = poison;
    }
    std::copy(dU.begin(), dU.end(), P_in);
    emu::launch((unsigned)((n_mat * ne + 255) / 256), 256, [&]() { hadi_jump_matrix_kernel(L, n_mat, vec_s, musig, G.data()); });
    for (int q = 0; q < n_mat; q++)
        emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_unpack_kernel(L, G.data() + (size_t)q * gd, G_out + (size_t)q * ne); });
    dUT = dU;  // U_temp <- U, then the sub-step out of place on the sub-batch alone
    const size_t so = (size_t)o * L.inst_stride;
    if (kernel == 0) {
        emu::launch(hadi_jump_grid(L, cnt, width), HADI_JUMP_THREADS, [&]() {
            hadi_jump_kernel(L, cnt, width, o, n_src, dUT.data() + so, dU.data() + so, G.data(), shared ? 0ll : (long long)gd, avec + o,
                             ipar.data() + o, 1);
        }, hadi_jump_smem(L));
    } else {
        const HadiJumpSel js{o, n_src, per, share, width};
        emu::launch(hadi_jump_sel_grid(L, js, cnt), HADI_JUMP_THREADS, [&]() {
            hadi_jump_sel_kernel(L, cnt, js, dUT.data() + so, dU.data() + so, G.data(), (long long)gd, avec + o, ipar.data() + o, 1);
        }, hadi_jump_smem(L));
    }
    std::copy(dU.begin(), dU.end(), P_out);
    emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U_out); });
    return 0;
}
