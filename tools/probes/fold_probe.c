/* Stray-write check of the host program builder (csrc/nf_host.hip) — CPU only, no handle, no GPU.
 *
 *     make -C noise_flow_amd/csrc fold_probe && tools/probes/fold_probe
 *
 * The Makefile target compiles nf_host.hip with -fsanitize=address,undefined on the host side and links it with the library's
 * other (unsanitised) objects into this stand-alone program.  Over a fixed list of (coupling width, H, W, flags) that reaches all
 * nine kernel paths in both directions it calls nf_fold_params, nf_fold_layout (size query, then an exactly-sized malloc buffer,
 * so that one float too many is a heap overflow the sanitizer reports), nf_cond_rows and nf_tile_segments, and — the gradient
 * blocks of nf_nll_grad, with and without NF_CFG_GRAD_MFMA — nf_grad_fold.  Three more layer lists hold every one of the 17 layer
 * kinds (csrc/nf_layers.h) between them, again with exactly sized parameter vectors, so a fold or a conditional layer that reads
 * past its block is reported.  Exit status 0 and the last line "fold_probe ok" = nothing reported, every path seen with a block in
 * both directions, both gradient blocks seen and every kind folded. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/noiseflow_hip.h"

#define N_PATHS 9
#define N_LAYERS 7
#define MAX_LAYERS 12

static uint32_t lcg_state = 12345u;
static float uniform(void) /* (-0.4, 0.4) */
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return ((float)(lcg_state >> 8) / 16777216.0f - 0.5f) * 0.8f;
}

static void permutation(float *q)
{
    static const int perm[4] = {2, 0, 3, 1};
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) q[r * 4 + c] = perm[r] == c ? 1.0f : 0.0f;
}

static float *make_model_of(const int32_t *types, int n_layers, int w, nf_layer_desc *layers, size_t *n_params)
{
    size_t n = 0;
    for (int i = 0; i < n_layers; ++i) {
        layers[i].type = types[i];
        layers[i].width = types[i] == NF_LAYER_COUPLING ? w : 0;
        layers[i].param_offset = (int64_t)n;
        const int64_t c = nf_layer_param_count(layers[i].type, layers[i].width);
        if (c < 0) return NULL;
        n += (size_t)c;
    }
    float *p = (float *)malloc(n * sizeof(float));   /* exactly sized: a read past the model is reported too */
    if (!p) return NULL;
    for (size_t i = 0; i < n; ++i) p[i] = uniform();
    for (int i = 0; i < n_layers; ++i) {
        float *q = p + layers[i].param_offset;
        if (types[i] == NF_LAYER_CONV1X1 || types[i] == NF_LAYER_CONV1X1_LU2) {   /* P, then sign_S (LU2: behind L) */
            permutation(q);
            for (int r = 0; r < 4; ++r) q[(types[i] == NF_LAYER_CONV1X1 ? 16 : 32) + r] = (r & 1) ? -1.0f : 1.0f;
        } else if (types[i] == NF_LAYER_CONV1X1_NONE) {
            for (int r = 0; r < 4; ++r) q[r * 5] += 2.0f;   /* diagonally dominant: not singular */
        } else if (types[i] == NF_LAYER_COUPLING) {
            for (int j = 0; j < w; ++j) {   /* the two batch-norm variances */
                q[20 * w + j] = 0.9f + uniform();
                q[23 * w + w * w + j] = 0.9f + uniform();
            }
        } else if (types[i] == NF_LAYER_GAIN4) {
            q[0] = 1.3f;
        }
    }
    *n_params = n;
    return p;
}

/* sdn | 1x1, coupling | gain4 | 1x1, coupling | gain: every op kind, two conditioning slots */
static float *make_model(int w, nf_layer_desc *layers, size_t *n_params)
{
    static const int32_t types[N_LAYERS] = {NF_LAYER_SDN, NF_LAYER_CONV1X1, NF_LAYER_COUPLING, NF_LAYER_GAIN4,
                                            NF_LAYER_CONV1X1, NF_LAYER_COUPLING, NF_LAYER_GAIN};
    return make_model_of(types, N_LAYERS, w, layers, n_params);
}

/* every layer kind in one of three lists (a model takes at most 4 conditional layers), folded in both directions at widths 4 and 5
 * and asked for its rows at every table ISO, an ISO outside the table and every camera */
static int vocabulary(void)
{
    static const struct { int n; int32_t t[MAX_LAYERS]; } lists[3] = {
        {11, {NF_LAYER_SDN5, NF_LAYER_CONV1X1, NF_LAYER_COUPLING, NF_LAYER_SDN4, NF_LAYER_CONV1X1_LU2, NF_LAYER_COUPLING, NF_LAYER_GAIN4,
              NF_LAYER_SDN1, NF_LAYER_PERMUTE, NF_LAYER_COUPLING, NF_LAYER_SDN2}},
        {7, {NF_LAYER_SDN3, NF_LAYER_CONV1X1_NONE, NF_LAYER_COUPLING, NF_LAYER_SDN6, NF_LAYER_GAIN1, NF_LAYER_COUPLING, NF_LAYER_GAIN2}},
        {4, {NF_LAYER_GAIN3, NF_LAYER_SDN, NF_LAYER_GAIN, NF_LAYER_COUPLING}},
    };
    static const nf_cond conds[6] = {{100.f, 0.f, 0.f, 0.f}, {400.f, 1.f, 0.f, 0.f}, {800.f, 2.f, 0.f, 0.f}, {1600.f, 3.f, 0.f, 0.f},
                                     {3200.f, 4.f, 0.f, 0.f}, {250.f, 0.f, 0.f, 0.f}};
    int kinds[NF_LAYER_PERMUTE + 1];
    memset(kinds, 0, sizeof(kinds));
    for (int k = 0; k < 3; ++k)
        for (int w = 4; w <= 5; ++w) {
            nf_layer_desc layers[MAX_LAYERS];
            size_t n_params = 0, n_folded = 0;
            float *params = make_model_of(lists[k].t, lists[k].n, w, layers, &n_params);
            if (!params) return 0;
            const nf_config cfg = {8, 8, 4, lists[k].n, -1, 0};
            for (int32_t direction = 0; direction < 2; ++direction) {
                int32_t n_ops = 0;
                double ld = 0.0;
                int rc = nf_fold_params(&cfg, layers, params, n_params, direction, NULL, 0, &n_ops, NULL, 0, &n_folded, &ld);
                if (rc == NF_OK) {
                    int32_t *ops = (int32_t *)malloc(2 * (size_t)n_ops * sizeof(int32_t));
                    float *blk = (float *)malloc(n_folded * sizeof(float));
                    nf_cond_row *rows = (nf_cond_row *)malloc(6 * sizeof(nf_cond_row));
                    rc = nf_fold_params(&cfg, layers, params, n_params, direction, ops, n_ops, &n_ops, blk, n_folded, &n_folded, &ld);
                    if (rc == NF_OK) rc = nf_cond_rows(&cfg, layers, params, n_params, direction, conds, 6, rows);
                    free(rows);
                    free(blk);
                    free(ops);
                }
                if (rc != NF_OK) {
                    fprintf(stderr, "vocabulary list %d width %d direction %d: %s\n", k, w, direction, nf_last_error());
                    return 0;
                }
            }
            for (int i = 0; i < lists[k].n; ++i) kinds[lists[k].t[i]]++;
            free(params);
        }
    for (int t = 1; t <= NF_LAYER_PERMUTE; ++t)
        if (!kinds[t]) {
            fprintf(stderr, "no vocabulary list holds layer kind %d\n", t);
            return 0;
        }
    printf("vocabulary: %d layer kinds folded\n", NF_LAYER_PERMUTE);
    return 1;
}

int main(void)
{
    static const int cases[][4] = {
        /* width, H, W, flags */
        {4, 32, 32, 0},   {4, 32, 32, NF_CFG_EXACT_FP32}, {4, 32, 32, NF_CFG_FP16_CNN}, {4, 64, 64, NF_CFG_FP16_CNN},
        {3, 5, 9, 0},     {4, 5, 9, NF_CFG_FP16_CNN},     {4, 128, 128, 0},             {4, 128, 128, NF_CFG_FP16_CNN},
        {6, 16, 16, 0},   {8, 50, 50, 0},                 {8, 64, 64, NF_CFG_FP16_CNN}, {8, 96, 80, 0},
        {12, 32, 32, 0},  {16, 64, 64, 0},                {16, 96, 80, NF_CFG_FP16_CNN}, {24, 32, 32, 0},
        {32, 64, 64, 0},  {32, 32, 32, NF_CFG_FP16_CNN},  {40, 16, 16, 0},              {40, 64, 64, 0},
        {40, 32, 32, NF_CFG_FP16_CNN}, {96, 32, 32, 0},   {96, 64, 64, NF_CFG_FP16_CNN}, {96, 128, 128, 0},
        {200, 32, 32, 0}, {200, 64, 64, NF_CFG_FP16_CNN}, {512, 32, 32, 0},             {512, 32, 32, NF_CFG_FP16_CNN},
    };
    int seen[2][N_PATHS];
    memset(seen, 0, sizeof(seen));
    long calls = 0;
    for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); ++k) {
        const int w = cases[k][0];
        nf_layer_desc layers[N_LAYERS];
        size_t n_params = 0;
        float *params = make_model(w, layers, &n_params);
        if (!params) {
            fprintf(stderr, "case %zu: no model\n", k);
            return 1;
        }
        nf_config cfg = {cases[k][1], cases[k][2], 4, N_LAYERS, -1, cases[k][3]};
        for (int32_t direction = 0; direction < 2; ++direction) {
            int32_t n_ops = 0;
            size_t n_folded = 0;
            double ld = 0.0;
            int rc = nf_fold_params(&cfg, layers, params, n_params, direction, NULL, 0, &n_ops, NULL, 0, &n_folded, &ld);
            if (rc != NF_OK) {
                fprintf(stderr, "case %zu (width %d, %dx%d, flags %d): nf_fold_params: %s\n", k, w, cfg.height, cfg.width, cfg.flags,
                        nf_last_error());
                return 1;
            }
            int32_t *ops = (int32_t *)malloc(2 * (size_t)n_ops * sizeof(int32_t));
            float *blk = (float *)malloc(n_folded * sizeof(float));
            rc = nf_fold_params(&cfg, layers, params, n_params, direction, ops, n_ops, &n_ops, blk, n_folded, &n_folded, &ld);
            free(blk);
            if (rc != NF_OK) return 1;
            for (int32_t path = 0; path < N_PATHS; ++path) {
                int32_t lw = 0;
                rc = nf_fold_layout(&cfg, layers, params, n_params, direction, path, NULL, 0, &n_ops, &lw, NULL, 0, &n_folded);
                ++calls;
                if (rc != NF_OK) continue;   /* this model has no block for the path */
                blk = (float *)malloc(n_folded * sizeof(float));
                rc = nf_fold_layout(&cfg, layers, params, n_params, direction, path, ops, n_ops, &n_ops, &lw, blk, n_folded, &n_folded);
                free(blk);
                if (rc != NF_OK) {
                    fprintf(stderr, "case %zu path %d: nf_fold_layout: %s\n", k, path, nf_last_error());
                    return 1;
                }
                seen[direction][path]++;
            }
            free(ops);
            const nf_cond conds[3] = {{100.f, 0.f, 0.f, 0.f}, {800.f, 2.f, 0.f, 0.f}, {3200.f, 4.f, 0.f, 0.f}};
            nf_cond_row *rows = (nf_cond_row *)malloc(3 * sizeof(nf_cond_row));
            rc = nf_cond_rows(&cfg, layers, params, n_params, direction, conds, 3, rows);
            free(rows);
            if (rc != NF_OK) {
                fprintf(stderr, "case %zu: nf_cond_rows: %s\n", k, nf_last_error());
                return 1;
            }
            const int ns = nf_tile_segments(&cfg, layers, params, n_params, direction, NULL, 0);
            if (ns < 0) return 1;
            int32_t *seg = (int32_t *)malloc((size_t)(ns > 0 ? ns : 1) * 5 * sizeof(int32_t));
            if (nf_tile_segments(&cfg, layers, params, n_params, direction, seg, ns) != ns) return 1;
            free(seg);
        }
        free(params);
    }
    /* the gradient blocks (nf_grad_fold): scalar layout, and the fetch-order layout of the matrix-core gradient kernel */
    static const int gcases[][4] = {{4, 32, 32, 0}, {8, 16, 16, NF_CFG_GRAD_MFMA}, {32, 16, 16, 0}, {32, 32, 32, NF_CFG_GRAD_MFMA},
                                    {24, 9, 13, NF_CFG_GRAD_MFMA}, {17, 1, 1, NF_CFG_GRAD_MFMA}};
    int gseen[2] = {0, 0};
    for (size_t k = 0; k < sizeof(gcases) / sizeof(gcases[0]); ++k) {
        nf_layer_desc layers[N_LAYERS];
        size_t n_params = 0, n_folded = 0;
        float *params = make_model(gcases[k][0], layers, &n_params);
        if (!params) return 1;
        nf_config cfg = {gcases[k][1], gcases[k][2], 4, N_LAYERS, -1, gcases[k][3]};
        int32_t n_ops = 0, gpath = -1;
        int rc = nf_grad_fold(&cfg, layers, params, n_params, &gpath, NULL, 0, &n_ops, NULL, 0, &n_folded);
        if (rc == NF_OK) {
            int32_t *ops = (int32_t *)malloc(2 * (size_t)n_ops * sizeof(int32_t));
            float *blk = (float *)malloc(n_folded * sizeof(float));
            rc = nf_grad_fold(&cfg, layers, params, n_params, &gpath, ops, n_ops, &n_ops, blk, n_folded, &n_folded);
            free(blk);
            free(ops);
        }
        if (rc != NF_OK || gpath < 0 || gpath > 1) {
            fprintf(stderr, "gradient case %zu: nf_grad_fold: %s\n", k, nf_last_error());
            return 1;
        }
        gseen[gpath]++;
        free(params);
    }
    printf("gradient blocks: %d scalar, %d matrix-core\n", gseen[0], gseen[1]);
    if (!gseen[0] || !gseen[1]) return 1;
    if (!vocabulary()) return 1;
    for (int d = 0; d < 2; ++d)
        for (int p = 0; p < N_PATHS; ++p) {
            printf("direction %d path %d: %d blocks\n", d, p, seen[d][p]);
            if (!seen[d][p]) {
                fprintf(stderr, "no case reached path %d in direction %d\n", p, d);
                return 1;
            }
        }
    printf("fold_probe ok (%ld nf_fold_layout queries)\n", calls);
    return 0;
}
