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
// Walker is a template over the TERRAIN MODE (include/ddrl_walker_hardcore.h): WalkerT<0> is the grass walker, whose
// instantiation is the code it was before the parameter existed (every addition below stands behind `if constexpr (HC)`, and the slot
// count NS folds to 8); WalkerT<1> is the HARDCORE terrain (stumps, pits, stairs: axis-aligned boxes in the state block behind row 286),
// specified by tests/walker_hardcore_oracle.py: 16 contact slots (corner q: floor slot 2 q, wall slot 2 q + 1), the hull's box test and
// the lidar's box edges.  The box of a corner is found through the per-column box index and loaded once per step, outside the sweeps.
// Internal linkage throughout, as env_device.h.
#pragma once
#include "env_device.h"

namespace {

constexpr int NFW = DDRL_ENVW_STATE_FIELDS;
enum { WPX = 14, WPY = 15, WL0 = 26, WJ0 = 50, WK0 = 70, WT0 = 86, WNT = 200, WNSEG = 13, WOBS = 24, WACT = 4 };
// the Hardcore block behind the grass walker's rows: wall-slot impulses, box count, box table (x0, x1, y0, y1), per-column box index
enum { WW0 = NFW, WNB = WW0 + 16, WB0 = WNB + 1, WMAXBOX = 40, WBC0 = WB0 + 4 * WMAXBOX, NFWH = WBC0 + WNT };
enum { WT_GRASS = 0, WT_STUMP, WT_STAIRS, WT_PIT, W_STARTPAD = 20, W_LAST_START = 173 };
enum { WFACE_NONE = 0, WFACE_TOP, WFACE_LEFT, WFACE_RIGHT };
constexpr uint32_t W_OBSTACLE_STEP0 = 0x08000000u;   // the obstacle draws of terrain point i: rng(W_OBSTACLE_STEP0 + i, 0..4)

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
constexpr float W_STEP4 = 4.0f * W_STEP;

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
constexpr int W_LDS_FIELDS_H = 16 * W_CFIELDS + 4 * W_JFIELDS;   // WalkerT<1>: 16 contact slots, 43 KiB per workgroup
// (the kernel declares `__shared__ float wl[WalkerT<HC>::LFIELDS][64]` and hands its lane's column to WalkerT::L)
// (LS: WalkerT's lane stride, 64 in every such kernel; a kernel that steps ONE env in one lane packs the fields at LS = 1)
#define WCF(f, s) L[((f) * NS + (s)) * LS]
#define WJF(f, j) L[(NS * W_CFIELDS + (f) * 4 + (j)) * LS]
// The compiler forwards a lane's own LDS stores to its later loads and hoists the loads out of the sweeps, which puts every field back
// into a register.  An empty statement that may touch memory, at the head of each sweep, makes it read the fields where they are.
#define W_LDS_FENCE() asm volatile("" ::: "memory")

__device__ __forceinline__ float signf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v); }

template <int HC, int LS = 64>
struct WalkerT {
    static constexpr int NS = HC ? 16 : 8;               // contact slots; slot s belongs to corner qof(s)
    static constexpr int LFIELDS = HC ? W_LDS_FIELDS_H : W_LDS_FIELDS;   // the floats of a lane's fields; its column spans LFIELDS * LS
    static __device__ constexpr int qof(int s) { return HC ? s >> 1 : s; }
    static __device__ constexpr int slot_row(int s) { return HC ? ((s & 1) ? WW0 : WK0) + 2 * (s >> 1) : WK0 + 2 * s; }
    float bx[5], by[5], ba[5], bvx[5], bvy[5], bom[5];   // bodies: centre of mass, angle, velocities
    float jpx[4], jpy[4], jm[4], jlo[4], jup[4];         // joint impulses (warm start)
    float can[NS], cat[NS];                              // contact impulses (warm start): corner q = 2 (body - 1) + k
    float px, py;                                        // hull origin
    float c1, c2, prev, hasp, eplen, epret, epi, pstep;
    float *L;                                            // this lane's column of the workgroup's LDS fields: field f at L[f * LS]
    float *Sc;                                           // this env's column of the state block: field f at Sc[f * n]
    float *T;                                            // ... and its terrain heights: T[k * n]
    float *B, *Cc;                                       // HC: its box table B[(4 b + f) * n] and per-column box index Cc[k * n]
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
    // HC: box `bi` of the table (an index out of a column's entry; false where that is none): its x0, x1, y0, y1
    __device__ bool box_at(float bi, float &x0, float &x1, float &y0, float &y1) const {
        if (!(bi >= 0.0f)) return false;
        const int b = min((int)bi, WMAXBOX - 1);   // (a set_state block may hold anything: never index past the table)
        const float *bp = B + (long long)(4 * b) * n;
        x0 = bp[0]; x1 = bp[n]; y0 = bp[2 * n]; y1 = bp[3 * n];
        return true;
    }
    // HC: the box index of column k, -1 for a column outside 0..199
    __device__ float box_index(int k) const { return (k < 0 || k > WNT - 1) ? -1.0f : Cc[(long long)k * n]; }
    // HC: the box consulted for a corner at (wx, wy) (oracle: WalkerHardcoreOracle._consult): its face, WFACE_NONE where no box is.
    // The three column entries are loaded together (independent loads: one round trip where no box is near, the common case), and a
    // neighbour column under the box the corner's own column holds is not looked at twice (it would fail the same test again).
    __device__ int consult(float wx, float wy, float &bx0, float &bx1, float &by1) const {
        const int kc = (int)clampf(floorf(wx / W_STEP), 0.0f, (float)(WNT - 2));
        const float bi[3] = {box_index(kc), box_index(kc - 1), box_index(kc + 1)};   // columns kc, kc - 1, kc + 1
        int face = WFACE_NONE;
        bx0 = bx1 = by1 = 0.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float x0, x1, y0, y1;
            if (face != WFACE_NONE || (d > 0 && bi[d] == bi[0]) || !box_at(bi[d], x0, x1, y0, y1)) continue;
            const float top = (wy - y1) - W_RADIUS, left = (x0 - wx) - W_RADIUS, right = (wx - x1) - W_RADIUS;
            if (top < 0.0f && left < 0.0f && right < 0.0f && y0 < wy) {
                face = (top >= left && top >= right) ? WFACE_TOP : (left >= right ? WFACE_LEFT : WFACE_RIGHT);
                bx0 = x0; bx1 = x1; by1 = y1;
            }
        }
        return face;
    }
    // b2EdgeShape::RayCast of the ten rays against the edge (v1x, v1y) + u (ex, ey), ee = ex ex + ey ey
    __device__ void ray10(float *f, const float *dx, const float *dy, float v1x, float v1y, float ex, float ey, float ee, bool valid) const {
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const float num = ey * (v1x - px) - ex * (v1y - py);
            const float den = ey * dx[i] - ex * dy[i];
            const float t = num / den;
            const float qx = px + t * dx[i], qy = py + t * dy[i];
            const float u = ((qx - v1x) * ex + (qy - v1y) * ey) / ee;
            const bool hit = valid && (den != 0.0f) && (t >= 0.0f) && (t <= 1.0f) && (u >= 0.0f) && (u <= 1.0f);
            f[i] = hit ? fminf(f[i], t) : f[i];
        }
    }
    // the ten lidar fractions (oracle: WalkerOracle.lidar; HC: WalkerHardcoreOracle.lidar)
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
        [[maybe_unused]] float prev_box = -1.0f;
        for (int m = 0; m < WNSEG; ++m) {
            const long long k1 = k0 + m + 1;
            const float hb = T[(k1 < WNT - 1 ? k1 : WNT - 1) * n];
            const bool valid = (k0 + m) <= WNT - 2;
            const float xa = (f0 + (float)m) * W_STEP;
            const float ey = hb - ha;
            ray10(f, dx, dy, xa, ha, W_STEP, ey, W_STEP2 + ey * ey, valid);
            if constexpr (HC) {
                // behind segment m: the three edges of its column's box, where that is another box than the previous column's
                const long long kcol = k0 + m < WNT - 1 ? k0 + m : WNT - 1;
                const float bi = Cc[kcol * n];
                float x0, x1, y0, y1;
                if (valid && bi != prev_box && box_at(bi, x0, x1, y0, y1)) {
                    const float w = x1 - x0, h = y1 - y0;
                    for (int e = 0; e < 3; ++e)   // top (x0, y1) + u (w, 0), left (x0, y0) + u (0, h), right (x1, y0) + u (0, h)
                        ray10(f, dx, dy, e == 2 ? x1 : x0, e == 0 ? y1 : y0, e == 0 ? w : 0.0f, e == 0 ? 0.0f : h, e == 0 ? w * w : h * h, true);
                }
                prev_box = bi;
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
    // contact slot s of body b, arm (rx, ry), corner (wx, wy), against the anchor (x0, h0) with normal (nx, ny): active flag (behind
    // `gate`), the fields the sweeps read, warm start
    __device__ __forceinline__ void init_slot(const int s, const int b, bool &on, const bool gate, const float rx, const float ry,
                                              const float wx, const float wy, const float x0, const float h0, const float nx, const float ny) {
        const float sep = ((wx - x0) * nx + (wy - h0) * ny) - W_RADIUS;
        on = gate && sep < 0.0f;
        can[s] = on ? can[s] : 0.0f;
        cat[s] = on ? cat[s] : 0.0f;
        const float tx = ny, ty = -nx;
        const float rn = rx * ny - ry * nx;
        const float rt = rx * ty - ry * tx;
        WCF(CRX, s) = rx; WCF(CRY, s) = ry; WCF(CNX, s) = nx; WCF(CNY, s) = ny; WCF(CX0, s) = x0; WCF(CH0, s) = h0;
        WCF(CNM, s) = 1.0f / (winvm(b) + winvi(b) * (rn * rn));
        WCF(CTM, s) = 1.0f / (winvm(b) + winvi(b) * (rt * rt));
        if (on) {
            const float Px = can[s] * nx + cat[s] * tx, Py = can[s] * ny + cat[s] * ty;
            bvx[b] = bvx[b] + winvm(b) * Px;
            bvy[b] = bvy[b] + winvm(b) * Py;
            bom[b] = bom[b] + winvi(b) * (rx * Py - ry * Px);
        }
    }
    // one physics step (oracle: WalkerOracle._physics; HC: WalkerHardcoreOracle._physics); returns the reward, sets done_env
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
        bool con[NS];
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
            if constexpr (!HC) {
                init_slot(q, b, con[q], true, rx, ry, wx, wy, x0, h0, nx, ny);
            } else {
                // floor slot: the terrain segment, or the consulted box's top; wall slot: the consulted box's side face
                float bx0, bx1, by1;
                const int face = consult(wx, wy, bx0, bx1, by1);
                const bool top = face == WFACE_TOP, left = face == WFACE_LEFT, side = face == WFACE_LEFT || face == WFACE_RIGHT;
                init_slot(2 * q, b, con[2 * q], true, rx, ry, wx, wy, top ? bx0 : x0, top ? by1 : h0, top ? 0.0f : nx, top ? 1.0f : ny);
                init_slot(2 * q + 1, b, con[2 * q + 1], side, rx, ry, wx, wy, left ? bx0 : bx1, by1, left ? -1.0f : 1.0f, 0.0f);
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
            for (int s = 0; s < NS; ++s) {
                const int b = 1 + qof(s) / 2;
                if (con[s]) {
                    const float rx = WCF(CRX, s), ry = WCF(CRY, s), nx = WCF(CNX, s), ny = WCF(CNY, s);
                    const float tx = ny, ty = -nx;
                    // tangent
                    float dvx = bvx[b] - bom[b] * ry;
                    float dvy = bvy[b] + bom[b] * rx;
                    float lam = WCF(CTM, s) * -(dvx * tx + dvy * ty);
                    const float lim = W_MU * can[s];
                    float nw = clampf(cat[s] + lam, -lim, lim);
                    lam = nw - cat[s];
                    cat[s] = nw;
                    float Px = lam * tx, Py = lam * ty;
                    bvx[b] = bvx[b] + winvm(b) * Px;
                    bvy[b] = bvy[b] + winvm(b) * Py;
                    bom[b] = bom[b] + winvi(b) * (rx * Py - ry * Px);
                    // normal
                    dvx = bvx[b] - bom[b] * ry;
                    dvy = bvy[b] + bom[b] * rx;
                    lam = -WCF(CNM, s) * (dvx * nx + dvy * ny);
                    nw = fmaxf(can[s] + lam, 0.0f);
                    lam = nw - can[s];
                    can[s] = nw;
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
            for (int s = 0; s < NS; ++s) {
                const int b = 1 + qof(s) / 2;
                if (con[s]) {
                    const float cx = (qof(s) & 1) ? whx(b) : -whx(b), cy = -W_HY;
                    const float nx = WCF(CNX, s), ny = WCF(CNY, s);
                    float sb, cb;
                    sincos32(ba[b], sb, cb);
                    const float qx = cb * cx - sb * cy, qy = sb * cx + cb * cy;
                    const float wx = bx[b] + qx, wy = by[b] + qy;
                    const float sep = ((wx - WCF(CX0, s)) * nx + (wy - WCF(CH0, s)) * ny) - W_RADIUS;
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
        if constexpr (!HC) {
            c1 = (con[2] || con[3]) ? 1.0f : 0.0f;
            c2 = (con[6] || con[7]) ? 1.0f : 0.0f;
        } else {   // either slot of a lower leg's corners
            c1 = (con[4] || con[5] || con[6] || con[7]) ? 1.0f : 0.0f;
            c2 = (con[12] || con[13] || con[14] || con[15]) ? 1.0f : 0.0f;
        }
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
            if constexpr (HC) {   // ... or strictly inside the box of its column
                float x0, x1, y0, y1;
                if (box_at(box_index((int)clampf(floorf(wx / W_STEP), 0.0f, (float)(WNT - 2))), x0, x1, y0, y1))
                    game_over = game_over || (wx > x0 && wx < x1 && wy > y0 && wy < y1);
            }
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
    // HC: randint(lo, hi) of a uniform draw; one box over the columns i0 .. i1 - 1 (the generator keeps i1 <= 199 and nb < WMAXBOX)
    static __device__ int randint(float u, int lo, int hi) { return lo + (int)fminf(floorf(u * (float)(hi - lo + 1)), (float)(hi - lo)); }
    __device__ void put_box(int &nb, int i0, int i1, float y0, float y1) {
        if (nb >= WMAXBOX || i0 < 0 || i1 > WNT - 1) return;   // (never taken: the bounds the generator keeps, held again at the store)
        float *bp = B + (long long)(4 * nb) * n;
        bp[0] = (float)i0 * W_STEP; bp[n] = (float)i1 * W_STEP; bp[2 * n] = y0; bp[3 * n] = y1;
        for (int k = i0; k < i1; ++k) Cc[(long long)k * n] = (float)nb;
        nb += 1;
    }
    // gym's terrain and body construction (oracle: WalkerOracle._build); env.reset() is build() + one zero-action physics()
    __device__ void build() {
        float y = W_TH, v = 0.0f;
        if constexpr (!HC) {
            for (int i = 0; i < WNT; ++i) {
                v = 0.8f * v + 0.01f * signf(W_TH - y);
                if (i > 20) v = v + (rng(RESET_STREAM, (uint32_t)i) * 2.0f - 1.0f) / SCALE;
                y = y + v;
                T[(long long)i * n] = y;
            }
        } else {
            // gym's _generate_terrain(hardcore=True) (oracle: WalkerHardcoreOracle._terrain1): GRASS / STUMP / STAIRS / PIT
            for (int f = WNB; f < WBC0; ++f) Sc[(long long)f * n] = 0.0f;
            for (int k = 0; k < WNT; ++k) Cc[(long long)k * n] = -1.0f;
            int state = WT_GRASS, counter = W_STARTPAD, nb = 0, sdir = 0, swidth = 0, ssteps = 0;
            bool oneshot = false;
            float oy = 0.0f;
            for (int i = 0; i < WNT; ++i) {
                const uint32_t ost = W_OBSTACLE_STEP0 + (uint32_t)i;
                if (state == WT_GRASS) {
                    v = 0.8f * v + 0.01f * signf(W_TH - y);
                    if (i > 20) v = v + (rng(RESET_STREAM, (uint32_t)i) * 2.0f - 1.0f) / SCALE;
                    y = y + v;
                } else if (state == WT_PIT && oneshot) {
                    const int c = randint(rng(ost, 2), 3, 5);
                    put_box(nb, i, i + 1, y - W_STEP4, y);
                    put_box(nb, i + c, i + c + 1, y - W_STEP4, y);
                    counter = c + 2;
                    oy = y;
                } else if (state == WT_PIT) {
                    y = oy;
                    if (counter > 1) y = y - W_STEP4;
                } else if (state == WT_STUMP && oneshot) {
                    const int c = randint(rng(ost, 2), 1, 3);
                    put_box(nb, i, i + c, y, y + (float)c * W_STEP);
                    counter = c;
                } else if (state == WT_STAIRS && oneshot) {
                    sdir = rng(ost, 2) > 0.5f ? 1 : -1;
                    swidth = randint(rng(ost, 3), 4, 5);
                    ssteps = randint(rng(ost, 4), 3, 5);
                    oy = y;
                    for (int s = 0; s < ssteps; ++s) {
                        const float top = y + (float)(s * sdir) * W_STEP;
                        put_box(nb, i + s * swidth, i + (s + 1) * swidth, top - W_STEP, top);
                    }
                    counter = ssteps * swidth;
                } else if (state == WT_STAIRS) {
                    const float nn = (float)(ssteps * swidth - counter - sdir) / (float)swidth;
                    y = oy + (nn * (float)sdir) * W_STEP;
                }
                oneshot = false;
                T[(long long)i * n] = y;
                counter -= 1;
                if (counter == 0) {
                    counter = randint(rng(ost, 0), 5, 10);
                    if (state == WT_GRASS && WMAXBOX - nb >= 5 && i + 1 <= W_LAST_START) {
                        state = 1 + randint(rng(ost, 1), 0, 2);
                        oneshot = true;
                    } else {
                        state = WT_GRASS;
                    }
                }
            }
            Sc[(long long)WNB * n] = (float)nb;
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
        for (int s = 0; s < NS; ++s) can[s] = cat[s] = 0.0f;
        c1 = c2 = prev = hasp = eplen = epret = pstep = 0.0f;
        // the fields no statement of the model sets (a set_state block may hold anything there)
        Sc[(long long)SLEEP * n] = 0.0f;
        for (int f = WPY + 1; f < PSTEP; ++f) Sc[(long long)f * n] = 0.0f;
    }
    __device__ void load(float *S, long long n_, long long i) {
        n = n_;
        Sc = S + i;
        T = Sc + (long long)WT0 * n;
        if constexpr (HC) { B = Sc + (long long)WB0 * n; Cc = Sc + (long long)WBC0 * n; }
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
        for (int s = 0; s < NS; ++s) {
            can[s] = S[(long long)slot_row(s) * n + i];
            cat[s] = S[(long long)(slot_row(s) + 1) * n + i];
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
        for (int s = 0; s < NS; ++s) {
            S[(long long)slot_row(s) * n + i] = can[s];
            S[(long long)(slot_row(s) + 1) * n + i] = cat[s];
        }
    }
};
using WalkerHardcore = WalkerT<1>;   // the Hardcore terrain at the step kernels' lane stride (walker.hip: WalkerT<HC>, HC = 1)
using WalkerHardcoreLane = WalkerT<1, 1>;   // walker_hardcore_eval.hip: one env in one lane, its 172 fields packed (688 bytes of LDS)

}  // namespace
