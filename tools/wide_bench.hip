// Dev harness for csrc/wide_l1.h: the wide layer-1 forward (split K + reduce) and wgrad kernels against a double-precision
// host loop at small ragged shapes, then timed at config 5's shape (batch 512, obs 28 224, hidden 400, three evaluations).
// hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form -Wno-unused-function tools/wide_bench.hip -o tools/wide_bench.bin
#include "../distributed-drl_amd/csrc/wide_l1.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static float *dev(const std::vector<float> &v) {
    float *p; hipMalloc(&p, v.size() * 4); hipMemcpy(p, v.data(), v.size() * 4, hipMemcpyHostToDevice); return p;
}
static std::vector<float> rnd(size_t n, float sc) {
    std::vector<float> v(n);
    for (auto &x : v) x = ((float)(rand() & 0xffff) / 32768.f - 1.f) * sc;
    return v;
}

static int WVF = 4, MNU = WD_NB;   // column units per tile (argv[1])
static const float *g_consts;
static int check(int nev, int M, int N, int K) {
    const int ldh = (N + 1 + 3) & ~3;
    std::vector<std::vector<float>> X(nev), W(nev), Bz(nev);
    WideArgs a{};
    wide_plan(a, nev, M, N, K, true, 4, 512, 32, MNU);
    float *part; hipMalloc(&part, wide_part_floats(a) * 4);
    std::vector<float *> H(nev);
    for (int e = 0; e < nev; ++e) {
        X[e] = rnd((size_t)M * K, 1.f); W[e] = rnd((size_t)K * N, 0.05f); Bz[e] = rnd(N, 0.5f);
        hipMalloc(&H[e], (size_t)M * ldh * 4); hipMemset(H[e], 0, (size_t)M * ldh * 4);
        a.ev[e] = WideEval{dev(X[e]), dev(W[e]), dev(Bz[e]), H[e], K};
    }
    a.part = part; a.a_rows = M; a.ldo = ldh; a.consts = g_consts;
    launch_wide_fwd(a, 0);
    hipDeviceSynchronize();
    double worst = 0;
    for (int e = 0; e < nev; ++e) {
        std::vector<float> h((size_t)M * ldh);
        hipMemcpy(h.data(), H[e], h.size() * 4, hipMemcpyDeviceToHost);
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < N; ++j) {
                double s = Bz[e][j];
                for (int k = 0; k < K; ++k) s += (double)X[e][(size_t)i * K + k] * W[e][(size_t)k * N + j];
                s = s > 0 ? s : 0;
                worst = std::max(worst, std::fabs(s - h[(size_t)i * ldh + j]) / (1.0 + std::fabs(s)));
            }
    }
    // wgrad: G = [X0 | 1]^T dZ
    std::vector<float> dZ = rnd((size_t)M * N, 0.1f);
    float *G; hipMalloc(&G, (size_t)(K + 1) * N * 4); hipMemset(G, 0xff, (size_t)(K + 1) * N * 4);
    WideArgs g{};
    wide_plan(g, 1, K + 1, N, M, false, 4, 0, 32, MNU);
    g.ev[0] = WideEval{a.ev[0].A, dev(dZ), nullptr, G, K}; g.a_rows = K; g.consts = g_consts;
    launch_wide_wgrad(g, 0);
    hipDeviceSynchronize();
    std::vector<float> hg((size_t)(K + 1) * N);
    hipMemcpy(hg.data(), G, hg.size() * 4, hipMemcpyDeviceToHost);
    double worst_g = 0;
    for (int i = 0; i <= K; i += (K > 4096 ? 97 : 1))
        for (int j = 0; j < N; ++j) {
            double s = 0;
            for (int k = 0; k < M; ++k) s += (double)(i < K ? X[0][(size_t)k * K + i] : 1.f) * dZ[(size_t)k * N + j];
            worst_g = std::max(worst_g, std::fabs(s - hg[(size_t)i * N + j]) / (1.0 + std::fabs(s)));
        }
    const bool ok = worst < 2e-5 && worst_g < 2e-5;
    printf("nev %d M %4d N %4d K %6d  S %2d/%2d: fwd err %.2e  wgrad err %.2e  %s (%s)\n", nev, M, N, K, a.S[0], a.S[1], worst, worst_g, ok ? "ok" : "MISMATCH",
           hipGetErrorString(hipGetLastError()));
    return ok ? 0 : 1;
}

// device-side fills of the byte-row arm: pseudo-random pixels, and the float32 image of the same values
__global__ void k_fill_u8(unsigned char *p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        unsigned x = (unsigned)i * 2654435761u + seed; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        p[i] = (unsigned char)(x >> 24);
    }
}
__global__ void k_u8_to_f32(const unsigned char *p, float *f, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) f[i] = (float)p[i];
}
// The forward on ring rows through an index list, float32 rows against the BYTES of the same rows (k_wide<true, 4, 32, true>): H1 must be
// bit-identical; then both timed, alternating, at config 5's shape out of `rows`-row arrays (random rows: far beyond the Infinity Cache).
static int u8_arm(int nev, int M, int N, int K, int rows, bool timed, const float *w, const float *wt, const float *bz) {
    const int ldh = (N + 1 + 3) & ~3;
    const size_t n = (size_t)rows * K;
    unsigned char *b1, *b2; float *f1, *f2, *hf, *hu, *part; long long *ridx;
    hipMalloc(&b1, n); hipMalloc(&b2, n); hipMalloc(&f1, n * 4); hipMalloc(&f2, n * 4);
    hipMalloc(&hf, (size_t)nev * M * ldh * 4); hipMalloc(&hu, (size_t)nev * M * ldh * 4); hipMalloc(&ridx, M * 8);
    k_fill_u8<<<4096, 256>>>(b1, n, 1u); k_fill_u8<<<4096, 256>>>(b2, n, 77u);
    k_u8_to_f32<<<4096, 256>>>(b1, f1, n); k_u8_to_f32<<<4096, 256>>>(b2, f2, n);
    std::vector<long long> ri(M);
    for (auto &r : ri) r = (long long)(((unsigned long long)rand() * 2654435761ull) % (unsigned long long)rows);
    ri[0] = rows - 1;
    hipMemcpy(ridx, ri.data(), M * 8, hipMemcpyHostToDevice);
    WideArgs a{};
    wide_plan(a, nev, M, N, K, true, 4, 512, 32, MNU);
    hipMalloc(&part, wide_part_floats(a) * 4);
    a.part = part; a.a_rows = M; a.ldo = ldh; a.consts = g_consts;
    WideArgs u = a;
    for (int e = 0; e < nev; ++e) {
        const float *W = e == 2 ? wt : w;
        a.ev[e] = WideEval{e ? f2 : f1, W, bz, hf + (size_t)e * M * ldh, K, ridx};
        u.ev[e] = WideEval{reinterpret_cast<const float *>(e ? b2 : b1), W, bz, hu + (size_t)e * M * ldh, K, ridx};
    }
    u.a_u8 = 1;
    hipMemset(hf, 0, (size_t)nev * M * ldh * 4); hipMemset(hu, 0xff, (size_t)nev * M * ldh * 4);
    launch_wide_fwd(a, 0); launch_wide_fwd(u, 0); hipDeviceSynchronize();
    std::vector<float> h0((size_t)nev * M * ldh), h1(h0.size());
    hipMemcpy(h0.data(), hf, h0.size() * 4, hipMemcpyDeviceToHost); hipMemcpy(h1.data(), hu, h1.size() * 4, hipMemcpyDeviceToHost);
    int diff = 0; double amax = 0;
    for (int e = 0; e < nev; ++e)
        for (int i = 0; i < M; ++i) {
            if (memcmp(&h0[((size_t)e * M + i) * ldh], &h1[((size_t)e * M + i) * ldh], N * 4)) ++diff;
            for (int j = 0; j < N; ++j) amax = std::max(amax, (double)h0[((size_t)e * M + i) * ldh + j]);
        }
    printf("byte rows: nev %d M %4d N %4d K %6d ring %6d rows: %d of %d H1 rows differ from the float32 rows' (max H1 %.3g)  %s (%s)\n", nev, M, N, K, rows,
           diff, nev * M, amax, diff || !(amax > 0) ? "MISMATCH" : "bit-identical", hipGetErrorString(hipGetLastError()));
    if (timed && !diff) {
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        float ms;
        for (int i = 0; i < 5; ++i) { launch_wide_fwd(a, 0); launch_wide_fwd(u, 0); }
        for (int rep = 0; rep < 5; ++rep)
            for (int v = 0; v < 2; ++v) {
                const WideArgs &x = v ? u : a;
                hipEventRecord(e0, 0);
                for (int i = 0; i < 20; ++i) launch_wide_fwd(x, 0);
                hipEventRecord(e1, 0); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
                printf("forward on ring rows (%d evaluations, %d workgroups) + reduce, %s A rows: %.1f us\n", nev, x.total, v ? "uint8  " : "float32", ms * 50.f);
            }
    }
    hipFree(b1); hipFree(b2); hipFree(f1); hipFree(f2); hipFree(hf); hipFree(hu); hipFree(part); hipFree(ridx);
    return diff || !(amax > 0) ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 1) MNU = atoi(argv[1]);
    if (wide_prepare() != hipSuccess) { printf("wide_prepare failed\n"); return 1; }
    g_consts = dev(std::vector<float>{1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
    int bad = 0;
    bad += check(3, 32, 400, 1024);
    bad += check(3, 50, 72, 1028);
    bad += check(5, 600, 100, 1040);
    bad += check(1, 512, 32, 2048);
    bad += check(3, 37, 400, 28224);
    if (bad) return 1;
    // timing at config 5's shape
    const int nev = 3, M = 512, N = 400, K = 28224, ldh = 404;
    WideArgs a{};
    wide_plan(a, nev, M, N, K, true, 4, 512, 32, MNU);
    float *x1, *x2, *w, *wt, *bz, *h, *part, *dz, *G;
    hipMalloc(&x1, (size_t)M * K * 4); hipMalloc(&x2, (size_t)M * K * 4); hipMalloc(&w, (size_t)K * N * 4); hipMalloc(&wt, (size_t)K * N * 4);
    hipMalloc(&bz, N * 4); hipMalloc(&h, (size_t)3 * M * ldh * 4); hipMalloc(&part, wide_part_floats(a) * 4); hipMalloc(&dz, (size_t)M * N * 4);
    hipMalloc(&G, (size_t)(K + 1) * N * 4);
    {   // random operands: zero-filled ones flatter the matrix pipes
        std::vector<float> t = rnd((size_t)M * K, 1.f);
        hipMemcpy(x1, t.data(), t.size() * 4, hipMemcpyHostToDevice); hipMemcpy(x2, t.data() + 1000, (t.size() - 1000) * 4, hipMemcpyHostToDevice);
        t = rnd((size_t)K * N, 0.05f);
        hipMemcpy(w, t.data(), t.size() * 4, hipMemcpyHostToDevice); hipMemcpy(wt, t.data() + 1000, (t.size() - 1000) * 4, hipMemcpyHostToDevice);
        t = rnd((size_t)M * N, 0.1f);
        hipMemcpy(dz, t.data(), t.size() * 4, hipMemcpyHostToDevice); hipMemset(bz, 0, N * 4);
    }
    a.ev[0] = WideEval{x1, w, bz, h, K}; a.ev[1] = WideEval{x2, w, bz, h + (size_t)M * ldh, K}; a.ev[2] = WideEval{x2, wt, bz, h + (size_t)2 * M * ldh, K};
    a.part = part; a.a_rows = M; a.ldo = ldh; a.consts = g_consts;
    WideArgs g{};
    wide_plan(g, 1, K + 1, N, M, false, 4, 0, 32, MNU);
    g.ev[0] = WideEval{x1, dz, nullptr, G, K}; g.a_rows = K; g.consts = g_consts;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float ms;
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0, 0);
        for (int i = 0; i < 10; ++i) launch_wide_fwd(a, 0);
        hipEventRecord(e1, 0); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
        printf("forward (3 evaluations, S = %d/%d, %d workgroups) + reduce: %.1f us  = %.1f TFLOP/s\n", a.S[0], a.S[1], a.total, ms * 100.f,
               2.0 * nev * M * N * (double)K / (ms * 1e-4) / 1e12);
        hipEventRecord(e0, 0);
        for (int i = 0; i < 10; ++i) launch_wide_wgrad(g, 0);
        hipEventRecord(e1, 0); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
        printf("wgrad (%d workgroups): %.1f us  = %.1f TFLOP/s\n", g.total, ms * 100.f, 2.0 * M * N * (double)(K + 1) / (ms * 1e-4) / 1e12);
    }
    {   // the forward on the bytes of compact-ring rows: ragged shapes (K % 32 == 16 tails, partial row blocks, narrow tiles), then config 5's
        std::vector<float> t = rnd((size_t)K * N, 0.0005f);
        hipMemcpy(w, t.data(), t.size() * 4, hipMemcpyHostToDevice); hipMemcpy(wt, t.data() + 1000, (t.size() - 1000) * 4, hipMemcpyHostToDevice);
        int ubad = 0;
        ubad += u8_arm(3, 37, 400, 1040, 300, false, w, wt, bz);
        ubad += u8_arm(5, 200, 48, 2064, 300, false, w, wt, bz);
        ubad += u8_arm(3, 96, 400, 1024, 300, false, w, wt, bz);
        ubad += u8_arm(3, M, N, K, 32768, true, w, wt, bz);
        if (ubad) return 1;
    }
    {   // race screen: the same launches 100 times, every output bit-identical to the first (LDS-DMA ordering is by vmcnt + barrier only)
        std::vector<float> h0((size_t)3 * M * ldh), h1(h0.size()), g0((size_t)(K + 1) * N), g1(g0.size());
        launch_wide_fwd(a, 0); launch_wide_wgrad(g, 0); hipDeviceSynchronize();
        hipMemcpy(h0.data(), h, h0.size() * 4, hipMemcpyDeviceToHost); hipMemcpy(g0.data(), G, g0.size() * 4, hipMemcpyDeviceToHost);
        int diff = 0;
        for (int it = 0; it < 100 && !diff; ++it) {
            hipMemsetAsync(h, 0xff, h0.size() * 4, 0); hipMemsetAsync(G, 0xff, g0.size() * 4, 0);
            launch_wide_fwd(a, 0); launch_wide_wgrad(g, 0); hipDeviceSynchronize();
            hipMemcpy(h1.data(), h, h1.size() * 4, hipMemcpyDeviceToHost); hipMemcpy(g1.data(), G, g1.size() * 4, hipMemcpyDeviceToHost);
            for (int e = 0; e < 3; ++e)
                for (int i = 0; i < M; ++i)
                    if (memcmp(&h0[((size_t)e * M + i) * ldh], &h1[((size_t)e * M + i) * ldh], N * 4)) { diff = 1 + it; break; }
            if (memcmp(g0.data(), g1.data(), g0.size() * 4)) diff = -(1 + it);
        }
        printf("race screen, 100 repeats of forward + wgrad at config 5's shape: %s (%d)\n", diff ? "OUTPUTS DIFFER" : "bit-identical", diff);
        if (diff) return 1;
    }
#ifdef WD_STAMPS
    {
        long long *st; hipMalloc(&st, (size_t)a.total * 8 * 8 * 8); hipMemset(st, 0, (size_t)a.total * 8 * 8 * 8);
        a.stamps = st;
        launch_wide_fwd(a, 0); hipDeviceSynchronize();
        std::vector<long long> hs((size_t)a.total * 8 * 8);
        hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost);
        for (int nu = 3; nu <= 4; ++nu) {
            double ph[6] = {0}; long long n = 0, stages = 0;
            for (int wg = 0; wg < a.total; ++wg)
                for (int w = 0; w < WVF; ++w) {
                    const long long *o = &hs[((size_t)wg * WVF + w) * 8];
                    if (o[7] != nu) continue;
                    ++n; stages += o[6];
                    for (int i = 0; i < 6; ++i) ph[i] += (double)o[i];
                }
            if (n) printf("forward NU %d: %lld waves, %.1f stages each; cycles per stage: top %.0f issue %.0f compute %.0f landed %.0f barrier %.0f\n", nu, n,
                          (double)stages / n, ph[0] / stages, ph[1] / stages, ph[2] / stages, ph[3] / stages, ph[4] / stages);
        }
    }
#endif
    {   // the stream-K wgrad (k_wide_sk): timing, and with -DWD_STAMPS the per-wave anatomy
        std::vector<SkFrag> fr;
        const int nwg = wide_plan_sk(g, 512, fr);
        printf("stream-K plan: %d workgroups\n", nwg);
        if (nwg > 1) {
            SkFrag *fr_d; float *slab; int *flag, *err_h;
            hipMalloc(&fr_d, fr.size() * sizeof(SkFrag)); hipMemcpy(fr_d, fr.data(), fr.size() * sizeof(SkFrag), hipMemcpyHostToDevice);
            hipMalloc(&slab, (size_t)nwg * 4 * WD_NB * 16 * 64 * 4); hipMalloc(&flag, (nwg + 1) * 4); hipHostMalloc(&err_h, 4, hipHostMallocMapped); *err_h = 0;
            SkArgs sa{}; sa.w = g; sa.frags = fr_d; sa.slab = slab; sa.flag = flag; sa.nwg = nwg; sa.err = err_h;
            int epoch = 0;
            auto run = [&]() { hipMemsetAsync(flag, 0, (nwg + 1) * 4, 0); sa.epoch = ++epoch; launch_wide_sk(sa, 0); };
            for (int rep = 0; rep < 3; ++rep) {
                hipEventRecord(e0, 0);
                for (int i = 0; i < 10; ++i) run();
                hipEventRecord(e1, 0); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
                printf("stream-K wgrad (%d workgroups, incl. a 2 KB flag memset per launch): %.1f us  = %.1f TFLOP/s\n", nwg, ms * 100.f, 2.0 * M * N * (double)(K + 1) / (ms * 1e-4) / 1e12);
            }
#ifdef WD_STAMPS
            long long *st; hipMalloc(&st, (size_t)nwg * 4 * 16 * 8); hipMemset(st, 0, (size_t)nwg * 4 * 16 * 8);
            sa.stamps = st;
            run(); hipDeviceSynchronize();
            std::vector<long long> hs((size_t)nwg * 4 * 16);
            hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost);
            double ph[8] = {0}, life = 0, stages = 0; long long tmin = 1ll << 62, tmax = 0, emin = 1ll << 62; int n = 0;
            for (int wgi = 0; wgi < nwg; ++wgi)
                for (int w = 0; w < 4; ++w) {
                    const long long *o = &hs[((size_t)wgi * 4 + w) * 16];
                    ++n; life += (double)(o[1] - o[0]); stages += (double)o[2];
                    tmin = std::min(tmin, o[0]); tmax = std::max(tmax, o[1]); emin = std::min(emin, o[1]);
                    for (int i = 0; i < 8; ++i) ph[i] += (double)o[3 + i];
                }
            // s_memtime counts at 100 MHz on this part: 1 tick = 10 ns
            printf("stream-K anatomy (mean per wave, in s_memtime ticks of 10 ns): lifetime %.0f, stages %.1f | set-up %.0f  fill %.0f  issue %.0f  compute %.0f  landed %.0f  barrier %.0f  publish %.0f  stores %.0f\n",
                   life / n, stages / n, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n, ph[4] / n, ph[5] / n, ph[6] / n, ph[7] / n);
            printf("launch span: first start -> last end %lld ticks; earliest end %lld ticks after the first start\n", tmax - tmin, emin - tmin);
#endif
        }
    }
    printf("%s\n", hipGetErrorString(hipGetLastError()));
    return 0;
}
