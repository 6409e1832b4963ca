// Dev harness: the whole SAC1 update of the direct-operand path inside a hipGraph (config-2 shape), timed, plus — in a
// -DDDRL_STAMPS build — the per-workgroup anatomy of every launch of the LAST update (cycle stamps of thread 0 and the
// 100 MHz real-time counter for the launch's dispatch ramp / tail), broken down per job of the k_dg launches and per job and side-output
// class of the k_dfwd launches (dfwd_classes).
// hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=16 -mllvm -amdgpu-mfma-vgpr-form
//       -Wno-unused-function [-DDDRL_STAMPS] tools/upd_bench.hip -o tools/upd_bench.bin
#include "../distributed-drl_amd/csrc/sac1.hip"
#include "../distributed-drl_amd/csrc/common.hip"
#include "../distributed-drl_amd/csrc/replay.hip"
#include <algorithm>
#include <cstring>

#ifdef DDRL_STAMPS
// Per job and class of a k_dfwd launch (k = phase): which workgroups carry the side outputs of their row tile, and when they end.  The tile
// of a workgroup is recomputed from k_dfwd's own formulas (both orders: XCD panels, and pack bit 30's dependent / stored runs); the class of
// a tile is the set of extras it carries beside the GEMM every tile does:
//   H  writes blocks of the H1r4 image (with their count)   X  the augmented input rows (aug / xr4)   N  the generated noise
//   S  the action / log-prob rows (DFJob::side)             T  the second policy_row of the `two` tile   st  stored-action evaluation
static void dfwd_classes(const ddrl_sac1_t *h, int k, const std::vector<unsigned long long> &hs, unsigned long long rmin) {
    const DFHead &H = k == 0 ? h->fh_a[0] : h->fh_b[0];
    const DFArgs &F = k == 0 ? h->f_a[0] : h->f_b[0];
    const int tiles_m = H.tiles_m, tpj = H.tpj, njobs = F.njobs, tiles_n = F.tiles_n, nwg = njobs * tpj;   // (the harness runs MT = 1)
    const int nblk = (H.K + 31) >> 5, bs = nblk >> 2, rem = nblk & 3;
    struct Cls { char name[24]; int n; double ssum, esum, emax, csum, cmax, p[6]; };
    for (int ji = 0; ji < njobs; ++ji) {
        std::vector<Cls> cls;
        for (int b = 0; b < nwg; ++b) {
            int t; bool stored = false;
            if (k == 1 && ((H.pack >> 30) & 1)) {
                const int nd = 3 * tpj, x = b & 7, slot = b >> 3, qd = nd >> 3, qs = (2 * tpj) >> 3;
                stored = slot >= qd;
                t = stored ? nd + x * qs + (slot - qd) : x * qd + slot;
            } else {
                const int q = nwg >> 3, r = nwg & 7, x = b & 7;
                t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
            }
            if (t / tpj != ji) continue;
            const int nt = (t - ji * tpj) / tiles_m;
            const DFJob &jb = F.job[ji];
            int nh = 0;
#ifdef DDRL_SIDE_SPREAD
            for (int w = 0; w < 4; ++w) {
                const int nb = bs + (w >= 4 - rem ? 1 : 0), b0 = w * bs + (w > 4 - rem ? w - (4 - rem) : 0);
                if (jb.H1r4) nh += __builtin_popcount(h1_owned(b0, nb, nt, tiles_n));
            }
            const bool X = (jb.aug || jb.xr4) && nt == side_aug_tile(tiles_n), N = k == 0 && F.noise_on && ji == 0 && nt == side_noise_tile(tiles_n);
#else   // before the side outputs were spread: everything on column tile 0
            if (jb.H1r4 && nt == 0) nh = nblk;
            const bool X = (jb.aug || jb.xr4) && nt == 0, N = k == 0 && F.noise_on && ji == 0 && nt == 0;
#endif
            const bool S = k == 1 && !stored && nt == 0 && jb.side != 0, T = k == 1 && ji == 1 && nt == 0 && F.php1 != nullptr;
            char name[24], hb[8] = "";
            if (nh) snprintf(hb, sizeof hb, "H%d", nh);
            snprintf(name, sizeof name, "%s%s%s%s%s%s", stored ? "st " : "", hb, X ? "X" : "", N ? "N" : "", S ? "S" : "", T ? "T" : "");
            if (!name[0] || !strcmp(name, "st ")) strcat(name, "rest");
            Cls *c = nullptr;
            for (auto &q : cls) if (!strcmp(q.name, name)) c = &q;
            if (!c) { cls.push_back(Cls{}); c = &cls.back(); strcpy(c->name, name); }
            const unsigned long long *p = &hs[((size_t)k * 1024 + b) * 16];
            if (!p[15]) continue;
            ++c->n; c->ssum += (p[14] - rmin) / 100.0;
            const double e = (p[15] - rmin) / 100.0; c->esum += e; c->emax = std::max(c->emax, e);
            const double cy = (double)(p[5] - p[0]); c->csum += cy; c->cmax = std::max(c->cmax, cy);
            for (int i = 1; i < 6; ++i) if (p[i] && p[i - 1]) c->p[i] += (double)(p[i] - p[i - 1]);
        }
        for (auto &c : cls)
            if (c.n) printf("      job %d %-10s: %3d wgs  start +%.2f us  end mean +%.2f max +%.2f us | cycles mean %.0f max %.0f | loads %.0f prol %.0f kloop %.0f bar %.0f epi %.0f\n", ji, c.name,
                            c.n, c.ssum / c.n, c.esum / c.n, c.emax, c.csum / c.n, c.cmax, c.p[1] / c.n, c.p[2] / c.n, c.p[3] / c.n, c.p[4] / c.n, c.p[5] / c.n);
    }
}
#endif

int main(int argc, char **argv) {
    const int per_graph = argc > 1 ? atoi(argv[1]) : 50;
    ddrl_sac1_config_t c{};
    c.obs_dim = 8; c.act_dim = 2; c.hidden1 = 400; c.hidden2 = 300; c.batch = 256; c.variant = DDRL_SAC1;
    c.alpha = 0.1; c.gamma = 0.997; c.lr = 5e-5; c.polyak = 0.995; c.beta1 = 0.9; c.beta2 = 0.999; c.adam_eps = 1e-8; c.act_scale = 1.0;
    ddrl_sac1_t *h = nullptr;
    if (ddrl_sac1_create(&h, 0, &c) != DDRL_OK) { printf("create failed: %s\n", ddrl_last_error()); return 1; }
    int64_t n_pi, n_q;
    ddrl_sac1_param_counts(&c, &n_pi, &n_q);
    const size_t n = (size_t)(n_pi + 2 * n_q);
    std::vector<float> w(n);
    srand(3);
    for (auto &v : w) v = ((float)(rand() & 0xffff) / 65536.f - 0.5f) * 0.1f;
    float *wd; hipMalloc(&wd, n * 4); hipMemcpy(wd, w.data(), n * 4, hipMemcpyHostToDevice);
    ddrl_sac1_set_weights(h, wd, nullptr);
    float *in[8];
    ddrl_sac1_input_buffers(h, 0, in);
    const int cnt[8] = {256 * 8, 256 * 8, 256 * 2, 256, 256, 256 * 2, 256 * 2, 256 * 2};
    for (int i = 0; i < 8; ++i) {
        std::vector<float> v(cnt[i]);
        for (auto &x : v) x = (float)(rand() & 0xffff) / 32768.f - 1.f;
        if (i == 4) for (auto &x : v) x = x > 0.9f ? 1.f : 0.f;
        hipMemcpy(in[i], v.data(), cnt[i] * 4, hipMemcpyHostToDevice);
    }
    hipStream_t s; hipStreamCreate(&s);
    auto one = [&]() { return ddrl_sac1_step(h, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], nullptr, nullptr, nullptr, nullptr, s); };
    for (int i = 0; i < 4; ++i) if (one() != DDRL_OK) { printf("step failed: %s\n", ddrl_last_error()); return 1; }
    hipStreamSynchronize(s);
    hipGraph_t g; hipGraphExec_t ge;
    hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    for (int i = 0; i < per_graph; ++i) one();
    ddrl_sac1_internal_opt_sync(h, s);
    hipStreamEndCapture(s, &g);
    if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) { printf("instantiate failed\n"); return 1; }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float ms, best = 1e9f;
    for (int rep = 0; rep < 6; ++rep) {
        hipEventRecord(e0, s);
        for (int k = 0; k < 4; ++k) hipGraphLaunch(ge, s);
        hipEventRecord(e1, s); hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        best = std::min(best, ms);
    }
    printf("graph of %d updates: %.2f us/update (%s)\n", per_graph, best * 1000.f / (4 * per_graph), hipGetErrorString(hipGetLastError()));
#ifdef DDRL_STAMPS
    unsigned long long *st;
    const size_t NS = (size_t)5 * 1024 * 16;
    hipMalloc(&st, NS * 8); hipMemset(st, 0, NS * 8);
    g_st_host = st;   // the stamp pointer travels in the kernel arguments: capture the same graph again, now stamped
    hipGraph_t g2; hipGraphExec_t ge2;
    hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    for (int i = 0; i < per_graph; ++i) one();
    ddrl_sac1_internal_opt_sync(h, s);
    hipStreamEndCapture(s, &g2);
    if (hipGraphInstantiate(&ge2, g2, nullptr, nullptr, 0) != hipSuccess) { printf("instantiate failed\n"); return 1; }
    hipGraphLaunch(ge2, s); hipStreamSynchronize(s);
    hipEventRecord(e0, s);
    for (int k = 0; k < 4; ++k) hipGraphLaunch(ge2, s);
    hipEventRecord(e1, s); hipEventSynchronize(e1);
    hipEventElapsedTime(&ms, e0, e1);
    printf("stamped graph: %.2f us/update\n", ms * 1000.f / (4 * per_graph));
    std::vector<unsigned long long> hs(NS);
    auto anatomy = [&](const char *title) {
    printf("---- %s\n", title);
    hipMemcpy(hs.data(), st, NS * 8, hipMemcpyDeviceToHost);
    const char *kn[5] = {"k_dfwd<0>", "k_dfwd<1>", "k_dg bq", "k_dg mid", "k_dg pi"};
    const char *pn[6] = {"", "loads-issued", "prologue", "k-loop", "combine-bar", "epilogue"};
    unsigned long long prev_end = 0;
    for (int k = 0; k < 5; ++k) {
        double ph[6] = {0}, tot = 0; int nwg = 0;
        unsigned long long rmin = ~0ull, rmax = 0, rstart_max = 0, lmax = 0;
        for (int b = 0; b < 1024; ++b) {
            const unsigned long long *p = &hs[((size_t)k * 1024 + b) * 16];
            if (!p[15]) continue;
            ++nwg;
            for (int i = 1; i < 6; ++i) if (p[i] && p[i - 1]) ph[i] += (double)(p[i] - p[i - 1]);
            tot += (double)(p[5] - p[0]);
            lmax = std::max(lmax, p[5] - p[0]);
            rmin = std::min(rmin, p[14]); rmax = std::max(rmax, p[15]); rstart_max = std::max(rstart_max, p[14]);
        }
        if (!nwg) continue;
        printf("%-10s %4d wgs | span %.2f us (first start -> last end), last start +%.2f us, gap from previous launch's end %.2f us | per-wg cycles:", kn[k], nwg,
               (rmax - rmin) / 100.0, (rstart_max - rmin) / 100.0, prev_end ? ((double)rmin - (double)prev_end) / 100.0 : 0.0);
        for (int i = 1; i < 6; ++i) printf(" %s=%.0f", pn[i], ph[i] / nwg);
        printf(" | mean total %.0f max %llu\n", tot / nwg, lmax);
        prev_end = rmax;
        // per job of a k_dg launch: when its workgroups start / end relative to the launch's first start (100 MHz real-time counter)
        if (k < 2) dfwd_classes(h, k, hs, rmin);
        const DGJobs *J = k == 2 ? &h->dg_bq[0] : (k == 3 ? &h->dg_mid : (k == 4 ? &h->dg_pi : nullptr));
        if (J) {
            const int nwgs = J->total_tiles;
            for (int ji = 0; ji < J->njobs; ++ji) {
                double ssum = 0, esum = 0, emax = 0, csum = 0, cmax = 0, psum[6] = {0}, gsum[4] = {0}; int n = 0, ngen = 0;
                for (int b = 0; b < nwgs; ++b) {
                    const int q = nwgs >> 3, r = nwgs & 7, x = b & 7;
                    const int t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
                    if (t < J->job[ji].tile_start || t >= J->job[ji].tile_start + J->job[ji].ntiles) continue;
                    const unsigned long long *p = &hs[((size_t)k * 1024 + b) * 16];
                    if (!p[15]) continue;
                    ++n; ssum += (p[14] - rmin) / 100.0; const double e = (p[15] - rmin) / 100.0; esum += e; emax = std::max(emax, e);
                    const double c = (double)(p[5] - p[0]); csum += c; cmax = std::max(cmax, c);
                    for (int i = 1; i < 6; ++i) if (p[i] && p[i - 1]) psum[i] += (double)(p[i] - p[i - 1]);
                    if (p[6] && p[7] && p[8]) {   // tiles with a generated A operand: the parts of their "loads" span
                        ++ngen; gsum[0] += (double)(p[6] - p[0]); gsum[1] += (double)(p[7] - p[6]); gsum[2] += (double)(p[8] - p[7]); gsum[3] += (double)(p[1] - p[8]);
                    }
                }
                if (n) printf("      job %d type %d M %4d N %4d K %4d: %3d wgs  start +%.2f us  end mean +%.2f max +%.2f us | cycles mean %.0f max %.0f | loads %.0f prol %.0f kloop %.0f bar %.0f epi %.0f\n", ji, J->job[ji].type,
                              J->job[ji].M, J->job[ji].N, J->job[ji].K, n, ssum / n, esum / n, emax, csum / n, cmax, psum[1] / n, psum[2] / n, psum[3] / n, psum[4] / n, psum[5] / n);
                if (ngen) printf("            generated operand: requests issued %.0f  arrived + row math %.0f  head kernels staged %.0f  to loads-issued %.0f\n", gsum[0] / ngen, gsum[1] / ngen, gsum[2] / ngen, gsum[3] / ngen);
            }
        }
    }
    };
    anatomy("inside the update sequence (graph)");
    // the same launches repeated back to back, WITHOUT the optimizer step in the epilogues (ddrl_sac1_stage_time): inputs stay in the L2s
    hipMemset(st, 0, NS * 8);
    for (int stg : {2, 5, 7, 8, 9}) { float ms2; ddrl_sac1_stage_time(h, stg, 40, &ms2, s); }
    hipStreamSynchronize(s);
    anatomy("each launch repeated back to back, no optimizer step");
#endif
    return 0;
}
