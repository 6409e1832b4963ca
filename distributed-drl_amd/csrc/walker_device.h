// The BIPEDAL WALKER (DDRL_ENV_WALKER): hull + two two-segment legs on four motorised revolute joints, the legs' far-end corners (feet
// and knees) against the 199 terrain segments, ten lidar rays, Box2D's island solve with run-time iteration counts.  Specification:
// tests/walker_oracle.py — every arithmetic statement of Walker mirrors one line of WalkerOracle._physics / _build / lidar (float32, one
// rounding per operation, no FMA contraction: -ffp-contract=off, write no fmaf here).  What is gym's, what is Box2D's structure and what
// is this build's own is said in that file's header; the model is unpinned against gym.
// One lane per env, one wave per workgroup.  The five bodies and the accumulated joint and contact impulses live in registers across the
// sweeps; what a sweep only READS — the eight contact points' arms, normals, segment origins and masses, the four joints' arms, point
// matrices, angles and motor settings — lives in LDS as [field][lane] (W_LDS_FIELDS below: lane = bank, so no access conflicts; 108 fields =
// 27 KiB per workgroup), written once per step by the lane that reads it, so no barrier is needed.  Every register array is indexed by
// unrolled constants only (a run-time index would move it to scratch memory).  The 200 terrain heights stay in the state block: a contact
// point or hull vertex loads the two heights of the segment under it once per step, outside the sweeps, and the lidar walks its 14
// heights once per step.
// Internal linkage throughout, as env_device.h.
#pragma once
#include "env_device.h"

namespace {

constexpr int NFW = DDRL_ENVW_STATE_FIELDS;
enum { WPX = 14, WPY = 15, WL0 = 26, WJ0 = 50, WK0 = 70, WT0 = 86, WNT = 200, WNSEG = 13, WOBS = 24, WACT = 4 };

// mass data: derivation in tests/walker_oracle.py
constexpr float W_STEP = 0.46666667f, W_STEP2 = W_STEP * W_STEP, W_TH = 3.3333333f, W_RANGE = 5.3333335f;
constexpr float W_LCX = -0.02003643f, W_LCY = -0.00564663f, W_INV_MH = 0.18442623f, W_INV_IH = 0.5001513f;
constexpr float W_INV_MU = 3.3088236f, W_INV_IU = 29.291225f, W_INV_ML = 4.1360292f, W_INV_IL = 37.318806f;
constexpr float W_HXU = 0.13333334f, W_HXL = 0.10666667f, W_HY = 0.56666666f;
constexpr float W_X0 = 4.6666665f, W_Y0 = 5.6f, W_YU = 5.3f, W_YL = 4.1666665f, W_LEG_A0 = 0.05f, W_XEND = 88.666664f;
constexpr float W_JAX_HIP = 0.02003643f, W_JAY_HIP = -0.26102003f, W_JBX = 0.0f, W_JBY = 0.56666666f;
constexpr float W_AXM_HIP = 1.0f / (W_INV_IH + W_INV_IU), W_AXM_KNEE = 1.0f / (W_INV_IU + W_INV_IL);
constexpr float W_MAX_MOTOR_IMP = 1.6f, W_FUEL = 0.028f, W_MU = 0.70710677f;
constexpr float W_RADIUS = 0.02f, W_SLOP3N = -0.015f, W_ASLOP = 0.034906585f, W_MAXLC = 0.2f, W_MAXAC = 0.13962634f, W_INV_DT = 50.0f;
constexpr int W_FORCE_J = 200;

// bodies: 0 hull, 1 upper leg 0, 2 lower leg 0, 3 upper leg 1, 4 lower leg 1; joint j: body A = wja(j), body B = j + 1
__device__ constexpr float winvm(int b) { return b == 0 ? W_INV_MH : ((b & 1) ? W_INV_MU : W_INV_ML); }
__device__ constexpr float winvi(int b) { return b == 0 ? W_INV_IH : ((b & 1) ? W_INV_IU : W_INV_IL); }
__device__ constexpr float whx(int b) { return (b & 1) ? W_HXU : W_HXL; }
__device__ constexpr int wja(int j) { return (j & 1) ? j : 0; }
__device__ constexpr float wjax(int j) { return (j & 1) ? 0.0f : W_JAX_HIP; }
__device__ constexpr float wjay(int j) { return (j & 1) ? -W_HY : W_JAY_HIP; }
__device__ constexpr float wlo(int j) { return (j & 1) ? -1.6f : -0.8f; }
__device__ constexpr float wup(int j) { return (j & 1) ? -0.1f : 1.1f; }
__device__ constexpr float wspeed(int j) { return (j & 1) ? 6.0f : 4.0f; }
__device__ constexpr float waxm(int j) { return (j & 1) ? W_AXM_KNEE : W_AXM_HIP; }

__constant__ float WHULLX[5] = {-1.0f, 0.2f, 1.1333333f, 1.1333333f, -1.0f};
__constant__ float WHULLY[5] = {0.3f, 0.3f, 0.033333335f, -0.26666668f, -0.26666668f};

// what the sweeps only read, [field][lane]
enum { CRX = 0, CRY, CNX, CNY, CX0, CH0, CNM, CTM, W_CFIELDS };
enum { RAX = 0, RAY, RBX, RBY, K11, K12, K22, IDET, JANG, MSPD, MMAX, W_JFIELDS };
constexpr int W_LDS_FIELDS = 8 * W_CFIELDS + 4 * W_JFIELDS;
// (the kernel declares `__shared__ float wl[W_LDS_FIELDS][64]` and hands its lane's column to Walker::L)
#define WCF(f, q) L[((f) * 8 + (q)) * 64]
#define WJF(f, j) L[(8 * W_CFIELDS + (f) * 4 + (j)) * 64]
// The compiler forwards a lane's own LDS stores to its later loads and hoists the loads out of the sweeps, which puts every field back
// into a register.  An empty statement that may touch memory, at the head of each sweep, makes it read the fields where they are.
#define W_LDS_FENCE() asm volatile("" ::: "memory")

__device__ __forceinline__ float signf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v); }

struct Walker {
    float bx[5], by[5], ba[5], bvx[5], bvy[5], bom[5];   // bodies: centre of mass, angle, velocities
    float jpx[4], jpy[4], jm[4], jlo[4], jup[4];         // joint impulses (warm start)
    float can[8], cat[8];                                // contact impulses (warm start): q = 2 (body - 1) + k
    float px, py;                                        // hull origin
    float c1, c2, prev, hasp, eplen, epret, epi, pstep;
    float *L;                                            // this lane's column of the workgroup's LDS fields: field f at L[f * 64]
    float *Sc;                                           // this env's column of the state block: field f at Sc[f * n]
    float *T;                                            // ... and its terrain heights: T[k * n]
    long long n;
    uint32_t seed, id;
    int vit, pit;

    __device__ float rng(uint32_t step, uint32_t j) const {
        const uint32_t seed_e = seed ^ ddrl::mix32((uint32_t)epi);
        uint32_t h = ddrl::mix32(seed_e ^ 0x9E3779B9u);
        h = ddrl::mix32(h + id * 0x85EBCA6Bu + 0x27D4EB2Fu);
        h = ddrl::mix32(h ^ ((step * 16u + j) * 0xC2B2AE35u + 0x165667B1u));
        return ddrl::u01(h);
    }
    // terrain segment under world x: its left end (x0, h0) and rise dh
    __device__ void segment(float wx, float &x0, float &h0, float &dh) const {
        const float fi = clampf(floorf(wx / W_STEP), 0.0f, (float)(WNT - 2));
        const long long idx = (long long)fi;
        const float a = T[idx * n], b = T[(idx + 1) * n];
        x0 = fi * W_STEP;
        h0 = a;
        dh = b - a;
    }
    __device__ float ground(float wx) const {
        float x0, h0, dh;
        segment(wx, x0, h0, dh);
        const float t = (wx - x0) / W_STEP;
        return h0 + dh * t;
    }
    // the ten lidar fractions (oracle: WalkerOracle.lidar)
    __device__ void lidar(float *f) const {
        const float f0 = clampf(floorf(px / W_STEP), 0.0f, (float)(WNT - 2));
        const long long k0 = (long long)f0;
        float dx[10], dy[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            float s, c;
            sincos32((1.5f * (float)i) / 10.0f, s, c);
            dx[i] = s * W_RANGE;
            dy[i] = -(c * W_RANGE);
            f[i] = 1.0f;
        }
        float ha = T[k0 * n];
        for (int m = 0; m < WNSEG; ++m) {
            const long long k1 = k0 + m + 1;
            const float hb = T[(k1 < WNT - 1 ? k1 : WNT - 1) * n];
            const bool valid = (k0 + m) <= WNT - 2;
            const float xa = (f0 + (float)m) * W_STEP;
            const float ey = hb - ha;
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const float num = ey * (xa - px) - W_STEP * (ha - py);
                const float den = ey * dx[i] - W_STEP * dy[i];
                const float t = num / den;
                const float qx = px + t * dx[i], qy = py + t * dy[i];
                const float u = ((qx - xa) * W_STEP + (qy - ha) * ey) / (W_STEP2 + ey * ey);
                const bool hit = valid && (den != 0.0f) && (t >= 0.0f) && (t <= 1.0f) && (u >= 0.0f) && (u <= 1.0f);
                f[i] = hit ? fminf(f[i], t) : f[i];
            }
            ha = hb;
        }
    }
    // observation 0..13 (the lidar fractions 14..23 are lidar()'s)
    __device__ void obs14(float *o) const {
        o[0] = ba[0];
        o[1] = 2.0f * bom[0] / FPS;
        o[2] = ((0.3f * bvx[0]) * 20.0f) / FPS;
        o[3] = ((0.3f * bvy[0]) * 13.333333f) / FPS;
#pragma unroll
        for (int leg = 0; leg < 2; ++leg) {
            const int hip = 2 * leg, knee = 2 * leg + 1;
            o[4 + 5 * leg] = ba[hip + 1] - ba[wja(hip)];
            o[5 + 5 * leg] = (bom[hip + 1] - bom[wja(hip)]) / wspeed(hip);
            o[6 + 5 * leg] = (ba[knee + 1] - ba[wja(knee)]) + 1.0f;
            o[7 + 5 * leg] = (bom[knee + 1] - bom[wja(knee)]) / wspeed(knee);
            o[8 + 5 * leg] = leg == 0 ? c1 : c2;
        }
    }
    __device__ void obs(float *o) const {
        obs14(o);
        lidar(o + 14);
    }
    // one physics step (oracle: WalkerOracle._physics); returns the reward, sets done_env
    __device__ float physics(const float *act, bool &done_env) {
        float mag[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mag[j] = clampf(fabsf(act[j]), 0.0f, 1.0f);
            WJF(MSPD, j) = wspeed(j) * signf(act[j]);
            WJF(MMAX, j) = W_MAX_MOTOR_IMP * mag[j];
        }
        // integrate velocities (gravity)
#pragma unroll
        for (int b = 0; b < 5; ++b) bvy[b] = bvy[b] + GRAV * DT;
        // ---- contacts: initialise and warm-start
        bool con[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int b = 1 + q / 2;
            float sb, cb;
            sincos32(ba[b], sb, cb);
            const float cx = (q & 1) ? whx(b) : -whx(b), cy = -W_HY;
            const float rx = cb * cx - sb * cy, ry = sb * cx + cb * cy;
            const float wx = bx[b] + rx, wy = by[b] + ry;
            float x0, h0, dh;
            segment(wx, x0, h0, dh);
            const float ln = sqrtf(dh * dh + W_STEP2);
            const float nx = -dh / ln, ny = W_STEP / ln;
            const float sep = ((wx - x0) * nx + (wy - h0) * ny) - W_RADIUS;
            con[q] = sep < 0.0f;
            can[q] = con[q] ? can[q] : 0.0f;
            cat[q] = con[q] ? cat[q] : 0.0f;
            const float tx = ny, ty = -nx;
            const float rn = rx * ny - ry * nx;
            const float rt = rx * ty - ry * tx;
            WCF(CRX, q) = rx; WCF(CRY, q) = ry; WCF(CNX, q) = nx; WCF(CNY, q) = ny; WCF(CX0, q) = x0; WCF(CH0, q) = h0;
            WCF(CNM, q) = 1.0f / (winvm(b) + winvi(b) * (rn * rn));
            WCF(CTM, q) = 1.0f / (winvm(b) + winvi(b) * (rt * rt));
            if (con[q]) {
                const float Px = can[q] * nx + cat[q] * tx, Py = can[q] * ny + cat[q] * ty;
                bvx[b] = bvx[b] + winvm(b) * Px;
                bvy[b] = bvy[b] + winvm(b) * Py;
                bom[b] = bom[b] + winvi(b) * (rx * Py - ry * Px);
            }
        }
        // ---- joints: initialise and warm-start
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int A = wja(j), B = j + 1;
            const float mA = winvm(A), iA = winvi(A), mB = winvm(B), iB = winvi(B);
            float sa, ca, sb, cb;
            sincos32(ba[A], sa, ca);
            sincos32(ba[B], sb, cb);
            const float rAx = ca * wjax(j) - sa * wjay(j), rAy = sa * wjax(j) + ca * wjay(j);
            const float rBx = cb * W_JBX - sb * W_JBY, rBy = sb * W_JBX + cb * W_JBY;
            const float k11 = ((mA + mB) + (rAy * rAy) * iA) + (rBy * rBy) * iB;
            const float k12 = (-(rAy * rAx) * iA) - (rBy * rBx) * iB;
            const float k22 = ((mA + mB) + (rAx * rAx) * iA) + (rBx * rBx) * iB;
            const float det = k11 * k22 - k12 * k12;
            WJF(RAX, j) = rAx; WJF(RAY, j) = rAy; WJF(RBX, j) = rBx; WJF(RBY, j) = rBy;
            WJF(K11, j) = k11; WJF(K12, j) = k12; WJF(K22, j) = k22;
            WJF(IDET, j) = det != 0.0f ? 1.0f / det : det;
            WJF(JANG, j) = ba[B] - ba[A];
            const float axial = (jm[j] + jlo[j]) - jup[j];
            bvx[A] = bvx[A] - mA * jpx[j];
            bvy[A] = bvy[A] - mA * jpy[j];
            bom[A] = bom[A] - iA * ((rAx * jpy[j] - rAy * jpx[j]) + axial);
            bvx[B] = bvx[B] + mB * jpx[j];
            bvy[B] = bvy[B] + mB * jpy[j];
            bom[B] = bom[B] + iB * ((rBx * jpy[j] - rBy * jpx[j]) + axial);
        }
        // ---- velocity sweeps: joints, then contacts
        for (int it = 0; it < vit; ++it) {
            W_LDS_FENCE();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int A = wja(j), B = j + 1;
                const float mA = winvm(A), iA = winvi(A), mB = winvm(B), iB = winvi(B);
                const float rAx = WJF(RAX, j), rAy = WJF(RAY, j), rBx = WJF(RBX, j), rBy = WJF(RBY, j);
                const float k11 = WJF(K11, j), k12 = WJF(K12, j), k22 = WJF(K22, j), idet = WJF(IDET, j), jang = WJF(JANG, j);
                const float mmax = WJF(MMAX, j);
                // motor
                float cdot = (bom[B] - bom[A]) - WJF(MSPD, j);
                float imp = -waxm(j) * cdot;
                const float old = jm[j];
                jm[j] = clampf(old + imp, -mmax, mmax);
                imp = jm[j] - old;
                bom[A] = bom[A] - iA * imp;
                bom[B] = bom[B] + iB * imp;
                // lower limit
                float C = jang - wlo(j);
                cdot = bom[B] - bom[A];
                imp = -waxm(j) * (cdot + fmaxf(C, 0.0f) * W_INV_DT);
                float nw = fmaxf(jlo[j] + imp, 0.0f);
                imp = nw - jlo[j];
                jlo[j] = nw;
                bom[A] = bom[A] - iA * imp;
                bom[B] = bom[B] + iB * imp;
                // upper limit
                C = wup(j) - jang;
                cdot = bom[A] - bom[B];
                imp = -waxm(j) * (cdot + fmaxf(C, 0.0f) * W_INV_DT);
                nw = fmaxf(jup[j] + imp, 0.0f);
                imp = nw - jup[j];
                jup[j] = nw;
                bom[A] = bom[A] + iA * imp;
                bom[B] = bom[B] - iB * imp;
                // point
                const float cdx = ((bvx[B] - bom[B] * rBy) - bvx[A]) + bom[A] * rAy;
                const float cdy = ((bvy[B] + bom[B] * rBx) - bvy[A]) - bom[A] * rAx;
                const float ex = -cdx, ey = -cdy;
                const float jx = idet * (k22 * ex - k12 * ey);
                const float jy = idet * (k11 * ey - k12 * ex);
                jpx[j] = jpx[j] + jx;
                jpy[j] = jpy[j] + jy;
                bvx[A] = bvx[A] - mA * jx;
                bvy[A] = bvy[A] - mA * jy;
                bom[A] = bom[A] - iA * (rAx * jy - rAy * jx);
                bvx[B] = bvx[B] + mB * jx;
                bvy[B] = bvy[B] + mB * jy;
                bom[B] = bom[B] + iB * (rBx * jy - rBy * jx);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int b = 1 + q / 2;
                if (con[q]) {
                    const float rx = WCF(CRX, q), ry = WCF(CRY, q), nx = WCF(CNX, q), ny = WCF(CNY, q);
                    const float tx = ny, ty = -nx;
                    // tangent
                    float dvx = bvx[b] - bom[b] * ry;
                    float dvy = bvy[b] + bom[b] * rx;
                    float lam = WCF(CTM, q) * -(dvx * tx + dvy * ty);
                    const float lim = W_MU * can[q];
                    float nw = clampf(cat[q] + lam, -lim, lim);
                    lam = nw - cat[q];
                    cat[q] = nw;
                    float Px = lam * tx, Py = lam * ty;
                    bvx[b] = bvx[b] + winvm(b) * Px;
                    bvy[b] = bvy[b] + winvm(b) * Py;
                    bom[b] = bom[b] + winvi(b) * (rx * Py - ry * Px);
                    // normal
                    dvx = bvx[b] - bom[b] * ry;
                    dvy = bvy[b] + bom[b] * rx;
                    lam = -WCF(CNM, q) * (dvx * nx + dvy * ny);
                    nw = fmaxf(can[q] + lam, 0.0f);
                    lam = nw - can[q];
                    can[q] = nw;
                    Px = lam * nx; Py = lam * ny;
                    bvx[b] = bvx[b] + winvm(b) * Px;
                    bvy[b] = bvy[b] + winvm(b) * Py;
                    bom[b] = bom[b] + winvi(b) * (rx * Py - ry * Px);
                }
            }
        }
        // ---- integrate positions
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            bx[b] = bx[b] + DT * bvx[b]; by[b] = by[b] + DT * bvy[b]; ba[b] = ba[b] + DT * bom[b];
        }
        // ---- position sweeps: contacts, then joints; a solved env leaves the loop (Box2D's per-island early exit: a per-lane branch)
        bool solved = false;
        for (int it = 0; it < pit && !solved; ++it) {
            W_LDS_FENCE();
            float minsep = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int b = 1 + q / 2;
                if (con[q]) {
                    const float cx = (q & 1) ? whx(b) : -whx(b), cy = -W_HY;
                    const float nx = WCF(CNX, q), ny = WCF(CNY, q);
                    float sb, cb;
                    sincos32(ba[b], sb, cb);
                    const float qx = cb * cx - sb * cy, qy = sb * cx + cb * cy;
                    const float wx = bx[b] + qx, wy = by[b] + qy;
                    const float sep = ((wx - WCF(CX0, q)) * nx + (wy - WCF(CH0, q)) * ny) - W_RADIUS;
                    minsep = fminf(minsep, sep);
                    const float C = clampf(BAUM * (sep + SLOP), -W_MAXLC, 0.0f);
                    const float rn = qx * ny - qy * nx;
                    const float K = winvm(b) + winvi(b) * (rn * rn);
                    const float imp = -C / K;
                    const float Px = imp * nx, Py = imp * ny;
                    bx[b] = bx[b] + winvm(b) * Px;
                    by[b] = by[b] + winvm(b) * Py;
                    ba[b] = ba[b] + winvi(b) * (qx * Py - qy * Px);
                }
            }
            bool jok = true;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int A = wja(j), B = j + 1;
                const float mA = winvm(A), iA = winvi(A), mB = winvm(B), iB = winvi(B);
                const float angle = ba[B] - ba[A];
                const float C = angle <= wlo(j) ? clampf((angle - wlo(j)) + W_ASLOP, -W_MAXAC, 0.0f)
                                                : (angle >= wup(j) ? clampf((angle - wup(j)) - W_ASLOP, 0.0f, W_MAXAC) : 0.0f);
                const float limp = -waxm(j) * C;
                float aang = ba[A] - iA * limp;
                float bang = ba[B] + iB * limp;
                float sa, ca, sb, cb;
                sincos32(aang, sa, ca);
                sincos32(bang, sb, cb);
                const float pAx = ca * wjax(j) - sa * wjay(j), pAy = sa * wjax(j) + ca * wjay(j);
                const float pBx = cb * W_JBX - sb * W_JBY, pBy = sb * W_JBX + cb * W_JBY;
                const float Cx = ((bx[B] + pBx) - bx[A]) - pAx;
                const float Cy = ((by[B] + pBy) - by[A]) - pAy;
                const float perr = sqrtf(Cx * Cx + Cy * Cy);
                const float a11 = ((mA + mB) + (pAy * pAy) * iA) + (pBy * pBy) * iB;
                const float a12 = (-(pAy * pAx) * iA) - (pBy * pBx) * iB;
                const float a22 = ((mA + mB) + (pAx * pAx) * iA) + (pBx * pBx) * iB;
                const float det = a11 * a22 - a12 * a12;
                const float id = det != 0.0f ? 1.0f / det : det;
                const float jx = -(id * (a22 * Cx - a12 * Cy));
                const float jy = -(id * (a11 * Cy - a12 * Cx));
                bx[A] = bx[A] - mA * jx;
                by[A] = by[A] - mA * jy;
                aang = aang - iA * (pAx * jy - pAy * jx);
                bx[B] = bx[B] + mB * jx;
                by[B] = by[B] + mB * jy;
                bang = bang + iB * (pBx * jy - pBy * jx);
                ba[A] = aang;
                ba[B] = bang;
                const float aerr = angle <= wlo(j) ? wlo(j) - angle : (angle >= wup(j) ? angle - wup(j) : 0.0f);
                jok = jok && (perr <= SLOP) && (aerr <= W_ASLOP);
            }
            solved = (minsep >= W_SLOP3N) && jok;
        }
        // ---- the step's flags, the hull origin at the new pose, game-over test on the hull vertices
        c1 = (con[2] || con[3]) ? 1.0f : 0.0f;
        c2 = (con[6] || con[7]) ? 1.0f : 0.0f;
        pstep = pstep + 1.0f;
        float sn, cs;
        sincos32(ba[0], sn, cs);
        px = bx[0] - (cs * W_LCX - sn * W_LCY);
        py = by[0] - (sn * W_LCX + cs * W_LCY);
        bool game_over = false;
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            const float hx = WHULLX[v], hy = WHULLY[v];
            const float wx = px + (cs * hx - sn * hy);
            const float wy = py + (sn * hx + cs * hy);
            game_over = game_over || (wy < ground(wx));
        }
        // shaping, reward (gym bipedal_walker.py semantics)
        const float shaping = (130.0f * px) / SCALE - 5.0f * fabsf(ba[0]);
        float rew = hasp > 0.0f ? shaping - prev : 0.0f;
        prev = shaping;
        hasp = 1.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) rew = rew - W_FUEL * mag[j];
        const bool neg_x = px < 0.0f, finish = px > W_XEND;
        rew = (game_over || neg_x) ? -100.0f : rew;
        done_env = game_over || neg_x || finish;
        return rew;
    }
    // gym's terrain (grass only) and body construction (oracle: WalkerOracle._build); env.reset() is build() + one zero-action physics()
    __device__ void build() {
        float y = W_TH, v = 0.0f;
        for (int i = 0; i < WNT; ++i) {
            v = 0.8f * v + 0.01f * signf(W_TH - y);
            if (i > 20) v = v + (rng(RESET_STREAM, (uint32_t)i) * 2.0f - 1.0f) / SCALE;
            y = y + v;
            T[(long long)i * n] = y;
        }
        const float fx = (rng(RESET_STREAM, W_FORCE_J) * 2.0f - 1.0f) * 5.0f;
        bx[0] = W_X0 + W_LCX; by[0] = W_Y0 + W_LCY; ba[0] = 0.0f;
        px = W_X0; py = W_Y0;
        bvx[0] = (fx * DT) * W_INV_MH; bvy[0] = 0.0f; bom[0] = 0.0f;
#pragma unroll
        for (int b = 1; b < 5; ++b) {
            bx[b] = W_X0; by[b] = (b & 1) ? W_YU : W_YL;
            ba[b] = (b & 1) ? (b <= 2 ? -W_LEG_A0 : W_LEG_A0) : 0.0f;
            bvx[b] = bvy[b] = bom[b] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) jpx[j] = jpy[j] = jm[j] = jlo[j] = jup[j] = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) can[q] = cat[q] = 0.0f;
        c1 = c2 = prev = hasp = eplen = epret = pstep = 0.0f;
        // the fields no statement of the model sets (a set_state block may hold anything there)
        Sc[(long long)SLEEP * n] = 0.0f;
        for (int f = WPY + 1; f < PSTEP; ++f) Sc[(long long)f * n] = 0.0f;
    }
    __device__ void load(float *S, long long n_, long long i) {
        n = n_;
        Sc = S + i;
        T = Sc + (long long)WT0 * n;
        bx[0] = S[X * n + i]; by[0] = S[Y * n + i]; bvx[0] = S[VX * n + i]; bvy[0] = S[VY * n + i]; ba[0] = S[ANG * n + i];
        bom[0] = S[OM * n + i]; c1 = S[C1 * n + i]; c2 = S[C2 * n + i]; prev = S[PREV * n + i]; hasp = S[HASP * n + i];
        eplen = S[EPLEN * n + i]; epret = S[EPRET * n + i]; epi = S[EPI * n + i];
        pstep = S[PSTEP * n + i]; px = S[WPX * n + i]; py = S[WPY * n + i];
#pragma unroll
        for (int b = 1; b < 5; ++b) {
            const float *L = S + (long long)(WL0 + 6 * (b - 1)) * n + i;
            bx[b] = L[0]; by[b] = L[n]; bvx[b] = L[2 * n]; bvy[b] = L[3 * n]; ba[b] = L[4 * n]; bom[b] = L[5 * n];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *J = S + (long long)(WJ0 + 5 * j) * n + i;
            jpx[j] = J[0]; jpy[j] = J[n]; jm[j] = J[2 * n]; jlo[j] = J[3 * n]; jup[j] = J[4 * n];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            can[q] = S[(long long)(WK0 + 2 * q) * n + i];
            cat[q] = S[(long long)(WK0 + 2 * q + 1) * n + i];
        }
    }
    // everything but the terrain (build() writes it in place) and the fields no statement sets (they stay as the block holds them)
    __device__ void store(float *S, long long i) const {
        S[X * n + i] = bx[0]; S[Y * n + i] = by[0]; S[VX * n + i] = bvx[0]; S[VY * n + i] = bvy[0]; S[ANG * n + i] = ba[0];
        S[OM * n + i] = bom[0]; S[C1 * n + i] = c1; S[C2 * n + i] = c2; S[PREV * n + i] = prev; S[HASP * n + i] = hasp;
        S[EPLEN * n + i] = eplen; S[EPRET * n + i] = epret; S[EPI * n + i] = epi;
        S[PSTEP * n + i] = pstep; S[WPX * n + i] = px; S[WPY * n + i] = py;
#pragma unroll
        for (int b = 1; b < 5; ++b) {
            float *L = S + (long long)(WL0 + 6 * (b - 1)) * n + i;
            L[0] = bx[b]; L[n] = by[b]; L[2 * n] = bvx[b]; L[3 * n] = bvy[b]; L[4 * n] = ba[b]; L[5 * n] = bom[b];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float *J = S + (long long)(WJ0 + 5 * j) * n + i;
            J[0] = jpx[j]; J[n] = jpy[j]; J[2 * n] = jm[j]; J[3 * n] = jlo[j]; J[4 * n] = jup[j];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            S[(long long)(WK0 + 2 * q) * n + i] = can[q];
            S[(long long)(WK0 + 2 * q + 1) * n + i] = cat[q];
        }
    }
};

}  // namespace
