/* Stray-write check of the trainer's create path up to its first device call (csrc/nf_train.hip: argument and layer-list
 * validation, the trainable-parameter mask, the step plan) — CPU only, never with a GPU.
 *
 *     make -C noise_flow_amd/csrc train_plan_probe && tools/probes/train_plan_probe
 *
 * The Makefile target compiles nf_train.hip with -fsanitize=address,undefined on the host side and links it with the library's
 * other (unsanitised) objects into this stand-alone program.  Without a device nf_trainer_create works through everything that
 * needs none — for a valid layer list that is the whole plan construction — and then fails at its first HIP call, which frees
 * the half-built handle through the one clean-up route.  Layer lists: every neighbour pattern the plan distinguishes (couplings
 * chained directly, behind one Conv2d1x1, behind two, cut by another layer; a Conv2d1x1 first / last; kMaxLayers layers; every
 * one of the 17 layer kinds in some list; exactly sized parameter vectors, so a mask write past a block is a heap overflow) and
 * every validation failure.
 * Exit status 0 and the last line "train_plan_probe ok" = nothing reported and every call ended as expected. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/noiseflow_hip.h"

#define MAXL 64
enum { C = NF_LAYER_COUPLING, M = NF_LAYER_CONV1X1, S = NF_LAYER_SDN5, G = NF_LAYER_GAIN4, P = NF_LAYER_PERMUTE, L2 = NF_LAYER_CONV1X1_LU2,
       N0 = NF_LAYER_CONV1X1_NONE, S0 = NF_LAYER_SDN, S1 = NF_LAYER_SDN1, S2 = NF_LAYER_SDN2, S3 = NF_LAYER_SDN3, S4 = NF_LAYER_SDN4,
       S6 = NF_LAYER_SDN6, G0 = NF_LAYER_GAIN, G1 = NF_LAYER_GAIN1, G2 = NF_LAYER_GAIN2, G3 = NF_LAYER_GAIN3 };

static int build(const int32_t *types, int n, int w, nf_layer_desc *layers, float **params, size_t *n_params)
{
    size_t tot = 0;
    for (int i = 0; i < n; ++i) {
        layers[i].type = types[i];
        layers[i].width = types[i] == C ? w : 0;
        layers[i].param_offset = (int64_t)tot;
        const int64_t c = nf_layer_param_count(layers[i].type, layers[i].width);
        if (c < 0) return 0;
        tot += (size_t)c;
    }
    *params = (float *)calloc(tot ? tot : 1, sizeof(float));   /* exactly sized */
    *n_params = tot;
    return *params != NULL;
}

/* want_einval: the call must be refused by the validation; else it must get past it (and fail at the first HIP call: no device) */
static int create(const char *what, const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int64_t max_batch,
                  int32_t opt, int want_einval)
{
    nf_trainer *t = NULL;
    const int rc = nf_trainer_create(cfg, layers, params, n_params, max_batch, opt, &t);
    if (rc == NF_OK) {   /* a device was found after all */
        nf_trainer_destroy(t);
        fprintf(stderr, "%s: created a trainer — this probe is for machines without a GPU\n", what);
        return 0;
    }
    if ((rc == NF_EINVAL) != (want_einval != 0) || t != NULL) {
        fprintf(stderr, "%s: status %d (%s), expected %s\n", what, rc, nf_last_error(), want_einval ? "NF_EINVAL" : "a HIP error");
        return 0;
    }
    return 1;
}

int main(void)
{
    static const struct { int n; int32_t t[12]; } lists[] = {
        {3, {C, C, C}},                         /* chained directly */
        {5, {C, M, C, M, C}},                   /* behind one Conv2d1x1 each */
        {5, {S, M, C, M, C}},                   /* the fold at the bottom */
        {6, {S, C, C, G, C, M}},                /* a chain cut by another layer; a Conv2d1x1 last */
        {4, {C, M, M, C}},                      /* two Conv2d1x1 between: not fusable, the upper one folded */
        {4, {M, C, P, C}},                      /* a Conv2d1x1 first; a permutation runs on the same kernels */
        {5, {C, L2, C, G, G}},
        {1, {C}}, {1, {M}}, {2, {S, G}},        /* one coupling; no coupling at all */
        {12, {S, M, C, M, C, M, C, G, M, C, M, C}},
        {9, {S0, N0, C, S1, C, S2, C, S3, G0}}, /* the rest of the vocabulary (csrc/nf_layers.h): every kind's mask, a block at the very end */
        {8, {S4, C, S6, C, G1, G2, C, G3}},
    };
    static const int widths[] = {4, 8, 5, 32, 96};
    int ok = 1, calls = 0;
    for (size_t k = 0; k < sizeof(lists) / sizeof(lists[0]); ++k)
        for (size_t wi = 0; wi < sizeof(widths) / sizeof(widths[0]); ++wi) {
            nf_layer_desc layers[MAXL];
            float *params;
            size_t n_params;
            if (!build(lists[k].t, lists[k].n, widths[wi], layers, &params, &n_params)) return 1;
            const nf_config cfg = {32, 32, 4, lists[k].n, (int32_t)(wi & 1) - 1, 0};   /* device -1 (current) and 0 */
            char what[64];
            snprintf(what, sizeof(what), "list %zu width %d", k, widths[wi]);
            ok &= create(what, &cfg, layers, params, n_params, 8, NF_OPT_ADAM, 0);
            ++calls;
            free(params);
        }
    {   /* kMaxLayers layers, alternating */
        int32_t t[MAXL];
        nf_layer_desc layers[MAXL];
        float *params;
        size_t n_params;
        for (int i = 0; i < MAXL; ++i) t[i] = (i & 1) ? C : M;
        if (!build(t, MAXL, 4, layers, &params, &n_params)) return 1;
        nf_config cfg = {10, 12, 4, MAXL, -1, 0};
        ok &= create("64 layers", &cfg, layers, params, n_params, 3, NF_OPT_MOMENTUM, 0);
        /* ---- the validation failures, on this list */
        nf_config bad = cfg;
        bad.channels = 3;
        ok &= create("channels", &bad, layers, params, n_params, 3, NF_OPT_ADAM, 1);
        bad = cfg; bad.height = 0;
        ok &= create("height", &bad, layers, params, n_params, 3, NF_OPT_ADAM, 1);
        bad = cfg; bad.flags = NF_CFG_FP16_CNN;
        ok &= create("flags", &bad, layers, params, n_params, 3, NF_OPT_ADAM, 1);
        bad = cfg; bad.n_layers = MAXL + 1;
        ok &= create("n_layers", &bad, layers, params, n_params, 3, NF_OPT_ADAM, 1);
        ok &= create("max_batch", &cfg, layers, params, n_params, 0, NF_OPT_ADAM, 1);
        ok &= create("optimizer", &cfg, layers, params, n_params, 3, 77, 1);
        ok &= create("short parameter vector", &cfg, layers, params, n_params - 1, 3, NF_OPT_ADAM, 1);
        ok &= create("null layers", &cfg, NULL, params, n_params, 3, NF_OPT_ADAM, 1);
        nf_layer_desc alt[MAXL];
        memcpy(alt, layers, sizeof(alt));
        alt[MAXL - 1].type = 9999;
        ok &= create("unknown layer type", &cfg, alt, params, n_params, 3, NF_OPT_ADAM, 1);
        memcpy(alt, layers, sizeof(alt));
        alt[5].param_offset = alt[3].param_offset;
        ok &= create("overlapping blocks", &cfg, alt, params, n_params, 3, NF_OPT_ADAM, 1);
        memcpy(alt, layers, sizeof(alt));
        alt[3].width = 8;   /* its block is sized for width 4: too short for 8, or a second width */
        ok &= create("two widths", &cfg, alt, params, n_params, 3, NF_OPT_ADAM, 1);
        memcpy(alt, layers, sizeof(alt));
        alt[1].width = 600;
        ok &= create("width beyond 512", &cfg, alt, params, n_params, 3, NF_OPT_ADAM, 1);
        calls += 13;
        free(params);
    }
    if (!ok) return 1;
    printf("train_plan_probe ok (%d nf_trainer_create calls)\n", calls);
    return 0;
}
