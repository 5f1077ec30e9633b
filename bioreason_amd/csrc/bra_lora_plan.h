// bra_lora_plan.h — host side shared by the masked LoRA entry points (k_lora.hip, k_wgrad.hip): the group description they
// accept, the walk over a group wider than one launch, and the table of kernel instantiations.  No device code.
#pragma once
#include "bra_dropout.h"

namespace bra {

// the (r, nt, R) contract of include/bioreason_hip.h, with p and the 32-bit element index of the hash (rows x cols = the masked operand)
inline bool lora_drop_ok(float p, long rows, long cols, int r, int nt, int R) {
    if (!(p >= 0.f && p < 1.f) || rows * cols >= (1l << 32) || nt < 1) return false;
    if (r == 32) return (R == 32 || R == 64 || R == 128) && nt <= R / 32;
    return (r == 8 || r == 16 || r == 64 || r == 128) && nt <= 3 && R == (nt * r + 63) / 64 * 64;
}

inline DropCfg make_cfg(float p, const unsigned* seeds, int n) {
    DropCfg d;
    d.thr16 = drop_threshold(p);
    d.inv_keep = 1.f / (1.f - p);
    for (int j = 0; j < 4; ++j) d.seed[j] = j < n ? seeds[j] : 0u;
    return d;
}

// one launch of down / wgrad: rank columns [c0, c0 + Rs) of the group, which hold targets [j0, j0 + nts) of rank r
struct LoraSlice { int r, c0, Rs, j0, nts; };

// f(slice) for every slice of <= 128 rank columns (LDS and accumulators of down and wgrad hold no more), until one returns non-zero.
// r >= 64: a slice holds whole targets (R = nt r); r <= 32: R <= 128, one slice with all targets.  Plain bra_wgrad_tn has no targets
// (r = nt = 0) and reads only (c0, Rs).  lora_up_drop does not slice: its sum over targets stays in fp32 registers until the single
// rounding, and only its dts / A fragments grow with the group (8 registers per 32 columns each).
template <class F>
inline int lora_for_slices(int r, int nt, int R, F&& f) {
    for (int c0 = 0; c0 < R; c0 += 128) {
        const int Rs = R - c0 < 128 ? R - c0 : 128;
        const int rc = f(LoraSlice{r, c0, Rs, r >= 64 ? c0 / r : 0, r >= 64 ? Rs / r : nt});
        if (rc) return rc;
    }
    return 0;
}

// X(condition on the slice s, RB, NL, TR, NT): the instantiations of lora_down_drop_kernel and wgrad_tn_kernel, first match wins
#define BRA_LORA_ROWS(X)                                                                                                     \
    X(s.r == 32 && s.Rs == 32, 1, 1, 32, 1)                                                                                  \
    X(s.r == 32 && s.Rs == 64 && s.nts == 1, 2, 1, 32, 1)                                                                    \
    X(s.r == 32 && s.Rs == 64 && s.nts == 2, 2, 2, 32, 2)                                                                    \
    X(s.r == 32 && s.Rs == 128 && s.nts == 3, 4, 3, 32, 3)                                                                   \
    /* nt = 4, and nt = 1 / 2 at R = 128 (a direct C call only): the padding blocks hold zeros, masking them is exact */     \
    X(s.r == 32 && s.Rs == 128, 4, 4, 32, 4)                                                                                 \
    X(s.r == 8 && s.nts == 1, 2, 1, 8, 1)                                                                                    \
    X(s.r == 8 && s.nts == 2, 2, 1, 8, 2)                                                                                    \
    X(s.r == 8 && s.nts == 3, 2, 1, 8, 3)                                                                                    \
    X(s.r == 16 && s.nts == 1, 2, 1, 16, 1)                                                                                  \
    X(s.r == 16 && s.nts == 2, 2, 1, 16, 2)                                                                                  \
    X(s.r == 16 && s.nts == 3, 2, 2, 16, 3)                                                                                  \
    X(s.r == 64 && s.Rs == 64, 2, 2, 64, 1)                                                                                  \
    X(s.r == 64 && s.Rs == 128, 4, 4, 64, 2)                                                                                 \
    X(s.r == 128, 4, 4, 128, 1)

}  // namespace bra
