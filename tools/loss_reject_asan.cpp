// Stand-alone walk of the rejection table of csrc/loss_eval.hip's entry points (the eight loss entry points, hwgat_kd_set,
// hwgat_eval_acc_bytes, hwgat_eval_accumulate): NULLs, bad offset, bad shape, unpaired target_b / lam, a pair without its
// buffers, a misaligned state, and which code wins when several arguments are wrong.  Every case returns before a launch,
// so the program runs on a machine without a GPU.  Meant for the host code under sanitizers, from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Isl-hwgat_amd/csrc \
//         -c sl-hwgat_amd/csrc/loss_eval.hip -o /tmp/loss_eval_san.o
//   hipcc --offload-arch=gfx950 -std=c++17 -fsanitize=address,undefined -Iinclude \
//         -x hip tools/loss_reject_asan.cpp -x none /tmp/loss_eval_san.o -o /tmp/loss_reject_asan && /tmp/loss_reject_asan
//
// It prints "<n> cases, 0 failed" and exits 0, or names the cases whose code differs; a sanitizer report ends it.
#include <cstdint>
#include <cstdio>
#include "hwgat_hip.h"

static int fails = 0, cases = 0;
#define EXPECT(call, code)                                                                 \
    do {                                                                                   \
        const long long got = (long long)(call);                                           \
        ++cases;                                                                           \
        if (got != (long long)(code)) { ++fails; printf("FAIL line %d: %s -> %lld, expected %lld\n", __LINE__, #call, got, (long long)(code)); } \
    } while (0)

int main() {
    alignas(16) static float f[64];
    alignas(16) static int64_t l[16];
    alignas(16) static int32_t i[16];
    alignas(16) static unsigned char raw[64];
    float *z = f, *u = f + 8, *lse = f + 16, *rl = f + 20, *loss = f + 24, *rlb = f + 28, *ls = f + 32, *lt = f + 36, *rk = f + 40,
          *kd = f + 44, *g = f + 48, *dz = f + 52, *lam = f + 56;
    int64_t *y = l, *yb = l + 4, *cor = l + 8, *ag = l + 9, *tc = l + 10;
    int32_t *n = i, *rank = i + 2, *pred = i + 4, *live = i + 6, *rankb = i + 8, *tp = i + 10;
    void* st = raw;
    void* st_odd = raw + 4;
    const int64_t B = 2;
    const int C = 3, E = HWGAT_EINVAL, S = HWGAT_ESHAPE;
    const int64_t BIG = 0x80000000ll;

    // sce
    EXPECT(hwgat_sce_fwd(nullptr, y, n, lse, rl, rank, pred, loss, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, nullptr, n, lse, rl, rank, pred, loss, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, y, n, nullptr, rl, rank, pred, loss, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, y, n, lse, nullptr, rank, pred, loss, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, y, n, lse, rl, nullptr, pred, loss, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, y, n, lse, rl, rank, nullptr, loss, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, y, n, lse, rl, rank, pred, nullptr, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_fwd(z, y, nullptr, lse, rl, rank, pred, loss, 0, C, 0.1f, nullptr), S);
    EXPECT(hwgat_sce_fwd(z, y, nullptr, lse, rl, rank, pred, loss, BIG, C, 0.1f, nullptr), S);
    EXPECT(hwgat_sce_fwd(z, y, nullptr, lse, rl, rank, pred, loss, B, 0, 0.1f, nullptr), S);
    EXPECT(hwgat_sce_fwd(z, y, nullptr, lse, rl, rank, pred, loss, B, 65537, 0.1f, nullptr), S);
    EXPECT(hwgat_sce_fwd(nullptr, y, nullptr, lse, rl, rank, pred, loss, 0, C, 0.1f, nullptr), E);       // NULL wins over shape
    EXPECT(hwgat_sce_bwd(nullptr, y, n, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_bwd(z, nullptr, n, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_bwd(z, y, n, nullptr, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_bwd(z, y, n, lse, nullptr, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_bwd(z, y, n, lse, g, nullptr, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_sce_bwd(z, y, n, lse, g, dz, -1, C, 0.1f, nullptr), S);
    EXPECT(hwgat_sce_bwd(z, y, n, lse, g, dz, B, -1, 0.1f, nullptr), S);

    // bsce
    EXPECT(hwgat_bsce_fwd(nullptr, y, n, 0, lse, rl, rank, pred, loss, cor, live, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_fwd(z, y, nullptr, 0, lse, rl, rank, pred, loss, cor, live, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_fwd(z, y, n, 0, lse, rl, rank, pred, loss, nullptr, live, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_fwd(z, y, n, 0, lse, rl, rank, pred, loss, cor, nullptr, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_fwd(z, y, n, -1, lse, rl, rank, pred, loss, cor, live, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_fwd(z, y, n, BIG, lse, rl, rank, pred, loss, cor, live, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_fwd(z, y, n, -1, lse, rl, rank, pred, loss, cor, live, 0, C, 0.1f, nullptr), E);   // offset wins over shape
    EXPECT(hwgat_bsce_fwd(z, y, n, 0, lse, rl, rank, pred, loss, cor, live, 0, C, 0.1f, nullptr), S);
    EXPECT(hwgat_bsce_fwd(z, y, n, 0, lse, rl, rank, pred, loss, cor, live, B, 65537, 0.1f, nullptr), S);
    EXPECT(hwgat_bsce_bwd(z, y, nullptr, 0, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_bwd(z, y, n, 0, nullptr, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_bwd(z, y, n, 0, lse, nullptr, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_bwd(z, y, n, 0, lse, g, nullptr, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_bwd(z, y, n, -5, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_bsce_bwd(z, y, n, 0, lse, g, dz, B, 0, 0.1f, nullptr), S);

    // mbsce
    EXPECT(hwgat_mbsce_fwd(z, y, nullptr, lam, n, 0, lse, rl, rank, pred, loss, cor, live, rlb, rankb, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_fwd(z, y, yb, nullptr, n, 0, lse, rl, rank, pred, loss, cor, live, rlb, rankb, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_fwd(z, y, yb, lam, n, 0, lse, rl, rank, pred, loss, cor, live, nullptr, rankb, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_fwd(z, y, yb, lam, n, 0, lse, rl, rank, pred, loss, cor, live, rlb, nullptr, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_fwd(z, y, yb, lam, n, -1, lse, rl, rank, pred, loss, cor, live, rlb, rankb, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_fwd(z, y, yb, lam, n, 0, lse, rl, rank, pred, loss, cor, live, rlb, rankb, 0, C, 0.1f, nullptr), S);
    EXPECT(hwgat_mbsce_bwd(z, y, nullptr, lam, n, 0, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_bwd(z, y, yb, nullptr, n, 0, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_bwd(z, y, yb, lam, nullptr, 0, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_bwd(z, y, yb, lam, n, BIG, lse, g, dz, B, C, 0.1f, nullptr), E);
    EXPECT(hwgat_mbsce_bwd(z, y, yb, lam, n, 0, lse, g, dz, B, 65537, 0.1f, nullptr), S);

    // kd: the state
    EXPECT(hwgat_kd_state_bytes(), 8);
    EXPECT(hwgat_kd_set(nullptr, 0.5f, 4.f, nullptr), E);
    EXPECT(hwgat_kd_set(st_odd, 0.5f, 4.f, nullptr), E);
    EXPECT(hwgat_kd_set(st, -0.1f, 4.f, nullptr), S);
    EXPECT(hwgat_kd_set(st, 1.1f, 4.f, nullptr), S);
    EXPECT(hwgat_kd_set(st, 0.5f, 0.1f, nullptr), S);
    EXPECT(hwgat_kd_set(st, 0.5f, 33.f, nullptr), S);
    EXPECT(hwgat_kd_set(st, 0.f / 0.f, 4.f, nullptr), S);
    EXPECT(hwgat_kd_set(st_odd, 2.f, 4.f, nullptr), E);                                                  // alignment wins
#define KD_FWD(zz, uu, yy, ybb, ll, nn, off, ss, rlbb, rkbb, lss, BB, CC) \
    hwgat_kd_fwd(zz, uu, yy, ybb, ll, nn, off, ss, lse, rl, rank, pred, loss, cor, live, rlbb, rkbb, lss, lt, rk, tp, kd, ag, tc, BB, CC, 0.1f, nullptr)
    EXPECT(KD_FWD(nullptr, u, y, yb, lam, n, 0, st, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, nullptr, y, yb, lam, n, 0, st, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, u, nullptr, yb, lam, n, 0, st, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, nullptr, 0, st, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, nullptr, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, st, rlb, rankb, nullptr, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, n, -1, st, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, nullptr, n, 0, st, rlb, rankb, ls, B, C), E);                             // unpaired
    EXPECT(KD_FWD(z, u, y, nullptr, lam, n, 0, st, rlb, rankb, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, st, nullptr, rankb, ls, B, C), E);                             // a pair needs its buffers
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, st, rlb, nullptr, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, st_odd, rlb, rankb, ls, B, C), E);                             // misaligned state
    EXPECT(KD_FWD(z, u, y, nullptr, nullptr, n, 0, st_odd, nullptr, nullptr, ls, B, C), E);
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, st_odd, rlb, rankb, ls, 0, C), E);                             // wins over shape
    EXPECT(KD_FWD(z, u, y, yb, lam, n, 0, st, rlb, rankb, ls, 0, C), S);
    EXPECT(KD_FWD(z, u, y, nullptr, nullptr, n, 0, st, nullptr, nullptr, ls, B, 65537), S);
#define KD_BWD(zz, uu, ybb, ll, nn, off, ss, lss, gg, BB, CC) \
    hwgat_kd_bwd(zz, uu, y, ybb, ll, nn, off, ss, lse, lss, lt, gg, dz, BB, CC, 0.1f, nullptr)
    EXPECT(KD_BWD(nullptr, u, yb, lam, n, 0, st, ls, g, B, C), E);
    EXPECT(KD_BWD(z, nullptr, yb, lam, n, 0, st, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, yb, lam, nullptr, 0, st, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, yb, lam, n, 0, nullptr, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, yb, lam, n, 0, st, nullptr, g, B, C), E);
    EXPECT(KD_BWD(z, u, yb, lam, n, 0, st, ls, nullptr, B, C), E);
    EXPECT(KD_BWD(z, u, yb, lam, n, BIG, st, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, yb, nullptr, n, 0, st, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, nullptr, lam, n, 0, st, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, yb, lam, n, 0, st_odd, ls, g, B, C), E);
    EXPECT(KD_BWD(z, u, nullptr, nullptr, n, 0, st_odd, ls, g, 0, C), E);
    EXPECT(KD_BWD(z, u, nullptr, nullptr, n, 0, st, ls, g, 0, C), S);
    EXPECT(KD_BWD(z, u, yb, lam, n, 0, st, ls, g, B, 0), S);

    // the accumulator
    EXPECT(hwgat_eval_acc_bytes(0, 5, 8), -1);
    EXPECT(hwgat_eval_acc_bytes(65537, 5, 8), -1);
    EXPECT(hwgat_eval_acc_bytes(7, -1, 8), -1);
    EXPECT(hwgat_eval_acc_bytes(7, 5, -1), -1);
    EXPECT(hwgat_eval_acc_bytes(7, 5, 8), 8 * (5 + 6 + 49 + 8));
    EXPECT(hwgat_eval_acc_bytes(65536, 0, 0), 8 * (5 + 1 + 65536ll * 65536));
    EXPECT(hwgat_eval_accumulate(nullptr, rl, rank, pred, y, loss, n, B, C, 5, 8, nullptr), E);
    EXPECT(hwgat_eval_accumulate(raw, rl, rank, pred, y, nullptr, n, B, C, 5, 8, nullptr), E);
    EXPECT(hwgat_eval_accumulate(raw, rl, rank, pred, y, loss, n, B, C, -1, 8, nullptr), E);
    EXPECT(hwgat_eval_accumulate(raw, rl, rank, pred, y, loss, n, B, C, 5, -1, nullptr), E);
    EXPECT(hwgat_eval_accumulate(raw, rl, rank, pred, y, loss, n, 0, C, 5, 8, nullptr), S);
    printf("%d cases, %d failed\n", cases, fails);
    return fails != 0;
}
