/* wide_driver.c -- the C oracle above 64 agents under AddressSanitizer / UndefinedBehaviorSanitizer.
 *
 * TEST INFRASTRUCTURE ONLY.  A stand-alone host program (`make -C oracle wide`, run by
 * tests/test_oracle_wide_cpu.py): oc_reset + a few oc_step at N = 65 and N = 256, E = 1, both env
 * variants, every output buffer heap-allocated at exactly its size so that a per-agent array of the
 * oracle that is not sized by N is a finding.  The agents stand on a 6 m lattice (closer than the 10 m
 * penalty range and the 15 m radar) so the per-agent O(N) loops all do work.  Exit 0 = no finding. */
#include "aac_oracle.c"

#include <stdio.h>

static uint64_t lcg = 0x2545F4914F6CDD1Dull;
static double urand(void) {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg >> 11) * (1.0 / 9007199254740992.0);
}

static int run(int variant, int N, const uint8_t *occ, int gw, int gh, const double *bound) {
    enum { E = 1, W = 4, STEPS = 3 };
    const int K = N - 1, D0 = variant ? 6 : 6 + 4 * K;
    const size_t EN = (size_t)E * N;
    oc_cfg cfg = {E, N, W, variant ? 1 : 2, 1, variant ? 0 : 1, variant ? 150 : 50, gw, gh,
                  {bound[0], bound[1], bound[2], bound[3]}, occ, 1, variant, variant ? 10.0 : 5.0};
    double *pos = calloc(EN * 2, 8), *vel = calloc(EN * 2, 8), *ppos = calloc(EN * 2, 8), *pvel = calloc(EN * 2, 8);
    double *goal = calloc(EN * 2, 8), *wp = calloc(EN * W * 2, 8), *start = calloc(EN * 2, 8);
    double *st = calloc(EN * 2, 8), *swp = calloc(EN * W * 2, 8);
    int32_t *cur = calloc(EN, 4), *wc = calloc(EN, 4), *wall = calloc(EN, 4), *stp = calloc(E, 4), *midx = calloc(E, 4);
    int32_t *scnt = calloc(EN, 4);
    uint8_t *reach = calloc(EN, 1);
    oc_state s = {pos, vel, ppos, pvel, goal, wp, cur, wc, reach, wall, stp, midx, start};
    float *own = calloc(EN * D0, 4), *radar = calloc(EN * NRAY, 4), *nei = calloc(EN * K * 6, 4);
    float *rew = calloc(EN, 4), *act = calloc(EN * 2, 4);
    uint8_t *done = calloc(EN, 1), *mask = calloc(EN, 1), *edone = calloc(E, 1), *bbc = calloc(E * 4, 1);
    double *tcpa = calloc(EN * K, 8), *dcpa = calloc(EN * K, 8);
    int32_t *cc = calloc(EN, 4), *cp = calloc(EN, 4);
    oc_out out = {own, radar, nei, rew, done, mask, edone, bbc, tcpa, dcpa, cc, cp};
    for (int i = 0; i < N; ++i) {           /* 16 x 16 lattice, 6 m apart, inside the bounds */
        st[2 * i] = bound[0] + 20.0 + 6.0 * (i % 16) + 0.25 * urand();
        st[2 * i + 1] = bound[2] + 15.0 + 6.0 * (i / 16) + 0.25 * urand();
        for (int k = 0; k < W; ++k) {
            swp[((size_t)i * W + k) * 2] = st[2 * i] + 8.0 * (k + 1);
            swp[((size_t)i * W + k) * 2 + 1] = st[2 * i + 1] + 3.0 * (k + 1);
        }
        scnt[i] = 2 + i % (W - 1);
    }
    oc_reset(&cfg, &s, NULL, st, swp, scnt, NULL, &out);
    int seen = 0, bad = 0;
    for (int t = 0; t < STEPS; ++t) {
        for (size_t k = 0; k < EN * 2; ++k) act[k] = (float)(2.0 * urand() - 1.0);
        oc_step(&cfg, &s, act, &out);
        for (int i = 0; i < N; ++i) {
            seen |= mask[i];
            bad += !(rew[i] == rew[i]);                       /* a reward read from past an array: NaN or junk */
            for (int r = 0; r < NRAY; ++r) bad += !(radar[i * NRAY + r] >= 0.0f && radar[i * NRAY + r] <= 15.0f);
        }
    }
    oc_reset(&cfg, &s, edone, st, swp, scnt, NULL, &out);
    free(pos); free(vel); free(ppos); free(pvel); free(goal); free(wp); free(start); free(st); free(swp);
    free(cur); free(wc); free(wall); free(stp); free(midx); free(scnt); free(reach); free(own); free(radar);
    free(nei); free(rew); free(act); free(done); free(mask); free(edone); free(bbc); free(tcpa); free(dcpa);
    free(cc); free(cp);
    if (bad) { fprintf(stderr, "variant %d N %d: %d values out of range\n", variant, N, bad); return 1; }
    printf("variant %d N %d: mask bits seen 0x%02x\n", variant, N, seen);
    return 0;
}

int main(void) {
    enum { GW = 23, GH = 13 };
    const double bound[4] = {455.0, 680.0, 255.0, 385.0};
    static uint8_t occ[GW * GH];
    for (int j = 2; j < 11; ++j) occ[6 * GH + j] = (j != 6);
    for (int j = 1; j < 9; ++j) occ[15 * GH + j] = 1;
    const int ns[2] = {65, 256};
    for (int variant = 0; variant < 2; ++variant)
        for (int k = 0; k < 2; ++k)
            if (run(variant, ns[k], occ, GW, GH, bound)) return 2;
    printf("wide oracle run ok\n");
    return 0;
}
