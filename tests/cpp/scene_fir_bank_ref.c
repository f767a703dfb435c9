/* The taps a bank set of the scene filter mix stands for (include/openpbso_amd.h "scene filter mix", BANK) as plain C: the
 * reference of the tests.  Compiled by tests/scene_fir_bank_model.py with -ffp-contract=off: every fmaf below is one.
 * bank [F][C][K], index / weight [N][J] (object-major) -> taps [C][N][K], the layout pbso_scene_fir_set takes. */
#include <math.h>
#include <stddef.h>

void scene_fir_bank_ref(const float *bank, int C, int K, int N, int J, const int *index, const float *weight, float *taps) {
    for (int c = 0; c < C; ++c)
        for (int o = 0; o < N; ++o)
            for (int k = 0; k < K; ++k) {
                float acc = 0.f;
                for (int j = 0; j < J; ++j)
                    acc = fmaf(weight[(size_t)o * J + j], bank[((size_t)index[(size_t)o * J + j] * C + c) * K + k], acc);
                taps[((size_t)c * N + o) * K + k] = acc;
            }
}
