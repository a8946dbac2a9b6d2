// Stand-alone check + timing of the block cyclic reduction solver (nlls_bcr.hip) against a CPU bordered-band LDL'.
// build: hipcc -O3 -std=c++20 --offload-arch=gfx950 -munsafe-fp-atomics -mllvm -amdgpu-mfma-vgpr-form -o tools/bcr/bcr_test tools/bcr/bcr_test.hip (__graft_entry__.build() does); run on the GPU box.
// bcr_test: the case list below; bcr_test n bw nbd [reps [level]]: that case alone (level: per-level backward launches); bcr_test list ...: several; bcr_test floor: the pivot floor on two singular unknowns.  Every case: x against the CPU, and x of the
// last of its repeated solves against x of the first, bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../nllssolver.jl_amd/csrc/nlls_bcr.hip"

using namespace nlls;

#define CHK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { printf("%s: %s\n", #expr, hipGetErrorString(e_)); return 1; } } while (0)

static double cpu_solve(int n, int bw, int nbd, int H, const std::vector<double>& Sb, std::vector<double>& x) {
    const int nbr = nbd + 1;
    std::vector<double> B(Sb.begin(), Sb.begin() + (size_t)n * H);
    std::vector<double> C((size_t)nbr * nbr);
    for (int i = 0; i < nbr * nbr; ++i) C[i] = Sb[(size_t)n * H + i];
    for (int j = 0; j < n; ++j) {
        double* cj = &B[(size_t)j * H]; const double d = cj[0];
        const int em = std::min(bw, n - 1 - j);
        for (int e = 1; e <= em; ++e) {
            const double l = cj[e] / d; double* ce = &B[(size_t)(j + e) * H];
            for (int e2 = e; e2 <= em; ++e2) ce[e2 - e] -= l * cj[e2];
            for (int q = 0; q < nbr; ++q) ce[bw + 1 + q] -= l * cj[bw + 1 + q];
        }
        for (int q = 0; q < nbd; ++q) { const double l = cj[bw + 1 + q] / d; for (int q2 = q; q2 < nbr; ++q2) C[q2 + nbr * q] -= l * cj[bw + 1 + q2]; }
    }
    std::vector<double> xb(nbd + 1, 0.0);
    for (int j = 0; j < nbd; ++j) { const double d = C[j + nbr * j];
        for (int c2 = j + 1; c2 < nbd; ++c2) { const double f = C[c2 + nbr * j] / d; for (int i = c2; i < nbr; ++i) C[i + nbr * c2] -= C[i + nbr * j] * f; }
        for (int i = j + 1; i < nbr; ++i) C[i + nbr * j] /= d; }
    for (int r = nbd - 1; r >= 0; --r) { double v = C[nbd + nbr * r]; for (int r2 = r + 1; r2 < nbd; ++r2) v -= C[r2 + nbr * r] * xb[r2]; xb[r] = v; }
    // note: after the LDL' above row nbd of C holds z = D^-1 L^-1 rhs
    x.assign(n + nbd, 0.0);
    for (int q = 0; q < nbd; ++q) x[n + q] = xb[q];
    for (int j = n - 1; j >= 0; --j) { const double* cj = &B[(size_t)j * H]; double v = cj[bw + 1 + nbd];
        const int em = std::min(bw, n - 1 - j);
        for (int e = 1; e <= em; ++e) v -= cj[e] * x[j + e];
        for (int q = 0; q < nbd; ++q) v -= cj[bw + 1 + q] * xb[q];
        x[j] = v / cj[0]; }
    return 0;
}

// sing (nsing of them): unknowns made singular and solved with the pivot floor on (relfloor > 0: the panel's FLOOR instantiation, the guarded re-factorisation of the tile that
// meets one).  An EXACTLY zero row, column and diagonal does not get there: a zero pivot makes the unguarded chain's tile NaN, NaN is above no floor, and the solve reports
// it (bcr_factor: "a NaN pivot is left alone").  So unknown u = sing[q] is singular the way a gauge direction is, by cancellation: u and u - 1 are cut off from everything
// else and form the block [1 1; 1 1 + 2^-40] with the consistent right-hand side (0.5, 0.5) -- the pivot of u is 2^-40 exactly, not zero, and below 1e-11 of its diagonal
// entry.  Expected: x_u = 0 exactly (dropped), x_{u-1} = 0.5 and every other unknown as the CPU's LDL' of the system without the unknowns u, every dropped pivot counted
// once per solve (status[4]), and the last solve bit for bit the first.
static int run_case(int n, int bw, int nbd, int reps, unsigned seed, bool level_backward = false, const int* sing = nullptr, int nsing = 0, double relfloor = 0.0) {
    const int H = bw + 1 + nbd + 1, nbr = nbd + 1;
    std::mt19937_64 rng(seed); std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> Sb((size_t)n * H + (size_t)nbr * nbr, 0.0);
    std::vector<double> rowsum(n + nbd, 0.0);
    for (int j = 0; j < n; ++j) for (int e = 1; e <= bw && j + e < n; ++e) { const double v = U(rng); Sb[(size_t)j * H + e] = v; rowsum[j] += std::fabs(v); rowsum[j + e] += std::fabs(v); }
    for (int j = 0; j < n; ++j) for (int q = 0; q < nbd; ++q) { const double v = 0.3 * U(rng); Sb[(size_t)j * H + bw + 1 + q] = v; rowsum[j] += std::fabs(v); rowsum[n + q] += std::fabs(v); }
    for (int j = 0; j < nbd; ++j) for (int i = j + 1; i < nbd; ++i) { const double v = U(rng); Sb[(size_t)n * H + i + nbr * j] = v; rowsum[n + i] += std::fabs(v); rowsum[n + j] += std::fabs(v); }
    for (int j = 0; j < n; ++j) { Sb[(size_t)j * H] = rowsum[j] * (0.6 + 0.2 * U(rng)) + 0.5; Sb[(size_t)j * H + bw + 1 + nbd] = U(rng); }   // (not diagonally dominant: 0.6 x)
    for (int j = 0; j < nbd; ++j) { Sb[(size_t)n * H + j + nbr * j] = rowsum[n + j] + 1.0; Sb[(size_t)n * H + nbd + nbr * j] = U(rng); }
    // make it safely positive definite: add a multiple of the identity found from Gershgorin
    for (int j = 0; j < n; ++j) Sb[(size_t)j * H] += 0.45 * rowsum[j];
    for (int q = 0; q < nsing; ++q) for (int u = sing[q] - 1; u <= sing[q]; ++u) {
        for (int c = 0; c < H; ++c) Sb[(size_t)u * H + c] = 0.0;                                              // column u below the diagonal, its border entries, its rhs
        for (int e = 1; e <= bw && u - e >= 0; ++e) Sb[(size_t)(u - e) * H + e] = 0.0; }                     // row u left of the diagonal
    for (int q = 0; q < nsing; ++q) { double* c0 = &Sb[(size_t)(sing[q] - 1) * H]; double* c1 = c0 + H;
        c0[0] = 1.0; c0[1] = 1.0; c1[0] = 1.0 + std::ldexp(1.0, -40); c0[bw + 1 + nbd] = 0.5; c1[bw + 1 + nbd] = 0.5; }
    std::vector<double> xc;
    {   std::vector<double> Sc = Sb;                                                                          // the system without them: x = 0 there, nothing else moves
        for (int q = 0; q < nsing; ++q) { double* c0 = &Sc[(size_t)(sing[q] - 1) * H]; double* c1 = c0 + H; c0[1] = 0.0; c1[0] = 1.0; c1[bw + 1 + nbd] = 0.0; }
        cpu_solve(n, bw, nbd, H, Sc, xc); }
    if (!BcrSolver::supports(n, bw, nbd)) { printf("case n=%d bw=%d nbd=%d: unsupported\n", n, bw, nbd); return 0; }
    BcrSolver S; std::string err;
    Switches sw{}; sw.bcr_level_backward = level_backward;       // (one backward launch per level instead of the fused one: NLLS_BCR_LEVEL_BACKWARD=1 of the library)
    if (S.build(n, bw, nbd, H, &err, sw) != 0) { printf("build failed: %s\n", err.c_str()); return 1; }
    if (grant_bcr_lds(S) != hipSuccess) { printf("LDS grant failed\n"); return 1; }
    double *dS, *dx; int* dst;
    CHK(hipMalloc(&dS, Sb.size() * 8)); CHK(hipMalloc(&dx, (n + nbd + 16) * 8)); CHK(hipMalloc(&dst, 512));
    CHK(hipMemcpy(dS, Sb.data(), Sb.size() * 8, hipMemcpyHostToDevice)); CHK(hipMemset(dst, 0, 512)); CHK(hipMemset(dx, 0, (n + nbd + 16) * 8));
    hipStream_t st; CHK(hipStreamCreate(&st));
    if (S.enqueue(st, dS, dx, dst, relfloor) != 0) { printf("enqueue failed\n"); return 1; }
    CHK(hipStreamSynchronize(st));
    std::vector<double> xg(n + nbd); int status[80];
    CHK(hipMemcpy(xg.data(), dx, (n + nbd) * 8, hipMemcpyDeviceToHost)); CHK(hipMemcpy(status, dst, 320, hipMemcpyDeviceToHost));
#ifdef BCR_STAMPS
    for (int w = 0; w < 2; ++w) { printf("   stamps wave %d:", w); for (int i = 0; i < 20; ++i) printf(" %d", status[16 + 20 * w + i]); printf("\n"); }
    printf("   arrivals at barrier B, J=0:"); for (int i = 0; i < 8; ++i) printf(" %d", status[56 + i]); printf("   J=1:"); for (int i = 0; i < 8; ++i) printf(" %d", status[64 + i]); printf("\n");
#endif
    if (const char* dump = getenv("BCR_TEST_DUMP")) { FILE* f = fopen(dump, "wb"); if (!f || fwrite(xg.data(), 8, xg.size(), f) != xg.size()) { printf("cannot write %s\n", dump); return 1; } fclose(f); }      // x of the first solve, raw: two builds compare with cmp
    double num = 0, den = 0; int worst = -1;
    for (int i = 0; i < n + nbd; ++i) { const double d = std::fabs(xg[i] - xc[i]); if (d > num || d != d) { num = d; worst = i; } den = std::max(den, std::fabs(xc[i])); }
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    int rc = 0;
    for (int i = 0; i < 3; ++i) rc |= S.enqueue(st, dS, dx, dst, relfloor);
    CHK(hipEventRecord(e0, st));
    for (int i = 0; i < reps - 1; ++i) rc |= S.enqueue(st, dS, dx, dst, relfloor);
    int dropped_before = 0;                                       // (status[4] adds up over the solves: the last solve's own count is the difference)
    if (nsing) { CHK(hipStreamSynchronize(st)); CHK(hipMemcpy(&dropped_before, dst + 4, 4, hipMemcpyDeviceToHost)); }
    rc |= S.enqueue(st, dS, dx, dst, relfloor);
    CHK(hipEventRecord(e1, st)); CHK(hipEventSynchronize(e1));
    float ms = 0; CHK(hipEventElapsedTime(&ms, e0, e1));
    // the same system solved again (3 + reps times): no atomics anywhere in the cyclic reduction, so x of the last solve must be x of the first, bit for bit, and the status still 0
    std::vector<double> xl(n + nbd); int status2[4];
    CHK(hipMemcpy(xl.data(), dx, (n + nbd) * 8, hipMemcpyDeviceToHost)); CHK(hipMemcpy(status2, dst, 16, hipMemcpyDeviceToHost));
    const bool same = memcmp(xl.data(), xg.data(), (size_t)(n + nbd) * 8) == 0;
    bool ok = num <= 1e-9 * den && status[0] == 0 && status2[0] == 0 && rc == 0 && same;
    if (nsing) {
        int dropped_all = 0; CHK(hipMemcpy(&dropped_all, dst + 4, 4, hipMemcpyDeviceToHost));
        bool zero = true; for (int q = 0; q < nsing; ++q) zero = zero && xg[sing[q]] == 0.0;
        const int d1 = status[4], dl = dropped_all - dropped_before;
        printf("   floor %.1e: dropped first=%d last=%d  x at the singular unknowns %s\n", relfloor, d1, dl, zero ? "zero" : "NOT ZERO");
        ok = ok && zero && d1 >= 1 && d1 == dl;
    }
    printf("case n=%5d bw=%3d nbd=%2d  N=%4d NT=%d levels=%2zu launches=%2d %s  err=%.3e (|x|=%.3e, worst %d) status=%d  repeat=%s  %.1f us/solve  %s\n",
           n, bw, nbd, S.N, S.NT, S.levels.size(), S.launches, S.fused_backward ? "fused" : "per-level", num, den, worst, status[0] | status2[0], same ? "identical" : "DIFFERS", 1e3 * ms / reps, ok ? "OK" : "FAIL");
    hipFree(dS); hipFree(dx); hipFree(dst); hipStreamDestroy(st);
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    int fails = 0;
    // bcr_test n bw nbd [reps [level]]: that case alone, "level" = one backward launch per level (the stamps of a -DBCR_STAMPS build are the first solve's; -DBCR_STAMP_M=<chain length> selects the level)
    // bcr_test list n bw nbd fused|level [n bw nbd fused|level ...]: those cases in one process, two timed solves each (tests/test_gpu_bcr_panel.py)
    if (argc >= 2 && !strcmp(argv[1], "list")) {
        if ((argc - 2) % 4 != 0 || argc < 6) { printf("usage: bcr_test list n bw nbd fused|level ...\n"); return 2; }
        for (int a = 2; a < argc; a += 4) fails += run_case(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), 2, 11 + a, !strcmp(argv[a + 3], "level"));
        printf(fails ? "FAILED %d\n" : "all ok\n", fails); return fails ? 1 : 0;
    }
    // bcr_test floor: NT = 4, N = 4, pivot floor 1e-11 (the library's), one dropped unknown in tile column 0 of an eliminated block (block 1) and one in its last tile column, both backward forms
    if (argc >= 2 && !strcmp(argv[1], "floor")) {
        const int sing[2] = {64 + 5, 64 + 48 + 9};
        for (int lvl = 0; lvl < 2; ++lvl) fails += run_case(256, 64, 0, 2, 11, lvl != 0, sing, 2, 1e-11);
        printf(fails ? "FAILED %d\n" : "all ok\n", fails); return fails ? 1 : 0;
    }
    if (argc >= 4) { const int rc = run_case(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), argc >= 5 ? atoi(argv[4]) : 200, 11, argc >= 6 && !strcmp(argv[5], "level")); printf(rc ? "FAILED\n" : "all ok\n"); return rc; }
    const int cases[][3] = {{16, 5, 0}, {80, 65, 0}, {81, 65, 0}, {160, 65, 0}, {200, 17, 3}, {128, 5, 0}, {333, 40, 1}, {600, 65, 0}, {1000, 80, 15},
                            {3000, 65, 1}, {6000, 65, 0}, {6000, 65, 2}, {60000, 65, 0}, {5000, 33, 0}, {777, 1, 0}, {4096, 64, 7}};
    unsigned seed = 1;
    for (auto& c : cases) fails += run_case(c[0], c[1], c[2], 20, seed++);
    printf(fails ? "FAILED %d\n" : "all ok\n", fails);
    return fails ? 1 : 0;
}
