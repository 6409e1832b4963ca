// The ARTICULATED lander (DDRL_ENV_ARTICULATED): hull + two legs on revolute joints, leg-corner contacts against the terrain segments,
// Box2D's island solve with run-time iteration counts.  Specification: tests/lander3_oracle.py — every arithmetic statement of Env3
// mirrors one line of Lander3Oracle._physics / reset (float32, one rounding per operation, no FMA contraction: -ffp-contract=off, write
// no fmaf here).  What is gym's, what is Box2D's structure and what is this build's own is said in that file's header.
// One lane per env; the three bodies, the joint rows and the eight contact points live in registers across the sweeps: every array below
// is indexed by unrolled constants only (a run-time index would move it to scratch memory), the terrain by Env::ground's select pattern.
// Internal linkage throughout, as env_device.h.
#pragma once
#include "env_device.h"

namespace {

constexpr int NF3 = DDRL_ENV3_STATE_FIELDS;
enum { L0 = 26, J0 = 38, K0 = 48, PX = 64, PY = 65 };

// mass data: derivation in tests/lander3_oracle.py
constexpr float INV_MH = 0.20761245f, INV_IH = 1.2757044f, LCY = 0.10130719f, INV_ML = 14.0625f, INV_IL = 558.36395f, AXM = 0.001786864f;
constexpr float LEG_HX = 0.06666667f, LEG_HY = 0.26666668f, ANCX = 0.6666667f, ANCY = 0.6f, LEG_X0 = 0.6666667f, LEG_A0 = 0.05f;
constexpr float MOTOR_SPEED = 0.3f, MAX_MOTOR_IMP = 0.8f, MU3 = 0.14142136f, RADIUS = 0.02f, SLOP3N = -0.015f, ASLOP = 0.034906585f;
constexpr float MAXLC = 0.2f, MAXAC = 0.13962634f, INV_DT = 50.0f, SLEEP_LIN2 = 0.0001f, SLEEP_ANG2 = 0.0012184697f;

struct Body3 {
    float x, y, ang, vx, vy, om;
};

struct Env3 {
    Body3 hull, leg[2];
    float jpx[2], jpy[2], jm[2], jlo[2], jup[2];   // joint impulses (warm start)
    float can[8], cat[8];                          // contact impulses (warm start): leg b, corner k at 4 b + k
    float px, py;                                  // hull origin
    float c1, c2, prev, hasp, eplen, epret, sleep, epi, pstep;
    float terr[11];
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
        const float fi = clampf(floorf(wx * 0.5f), 0.0f, 9.0f);
        const int idx = (int)fi;
        float a = terr[0], b = terr[1];
#pragma unroll
        for (int i = 1; i < 10; ++i)
            if (idx == i) { a = terr[i]; b = terr[i + 1]; }
        x0 = 2.0f * fi;
        h0 = a;
        dh = b - a;
    }
    __device__ float ground(float wx) const {
        float x0, h0, dh;
        segment(wx, x0, h0, dh);
        const float t = (wx - x0) * 0.5f;
        return h0 + dh * t;
    }
    __device__ void obs(float *o) const {
        o[0] = (px - 10.0f) / 10.0f;
        o[1] = (py - (HELIPAD_Y + LEG_DOWN)) / 6.6666665f;
        o[2] = hull.vx * 10.0f / FPS;
        o[3] = hull.vy * 6.6666665f / FPS;
        o[4] = hull.ang;
        o[5] = 20.0f * hull.om / FPS;
        o[6] = c1;
        o[7] = c2;
    }
    // one physics step (oracle: Lander3Oracle._physics); returns the reward, sets done_env and o[8]
    __device__ float physics(float act0, float act1, bool &done_env, float *o) {
        const float a0 = clampf(act0, -1.0f, 1.0f), a1 = clampf(act1, -1.0f, 1.0f);
        const uint32_t step = (uint32_t)pstep;
        const float d0 = (rng(step, 0) * 2.0f - 1.0f) / SCALE;
        const float d1 = (rng(step, 1) * 2.0f - 1.0f) / SCALE;
        float sn, cs;
        sincos32(hull.ang, sn, cs);
        const float tip0 = sn, tip1 = cs, side0 = -tip1, side1 = tip0;
        const float lx = -(sn * LCY), ly = cs * LCY;
        // main engine
        const float m_power = a0 > 0.0f ? (clampf(a0, 0.0f, 1.0f) + 1.0f) * 0.5f : 0.0f;
        float ox = tip0 * (0.13333334f + 2.0f * d0) + side0 * d1;
        float oy = -tip1 * (0.13333334f + 2.0f * d0) - side1 * d1;
        float ix = -ox * MAIN_POWER * m_power, iy = -oy * MAIN_POWER * m_power;
        float rx = ox - lx, ry = oy - ly;
        hull.vx = hull.vx + ix * INV_MH;
        hull.vy = hull.vy + iy * INV_MH;
        hull.om = hull.om + (rx * iy - ry * ix) * INV_IH;
        // side engines
        const float direction = a1 < 0.0f ? -1.0f : 1.0f;
        const float s_power = fabsf(a1) > 0.5f ? clampf(fabsf(a1), 0.5f, 1.0f) : 0.0f;
        const float arm = 3.0f * d1 + direction * SIDE_AWAY;
        ox = tip0 * d0 + side0 * arm;
        oy = -tip1 * d0 - side1 * arm;
        ix = -ox * SIDE_POWER * s_power; iy = -oy * SIDE_POWER * s_power;
        rx = (ox - tip0 * 0.56666666f) - lx;
        ry = (oy + tip1 * SIDE_H) - ly;
        hull.vx = hull.vx + ix * INV_MH;
        hull.vy = hull.vy + iy * INV_MH;
        hull.om = hull.om + (rx * iy - ry * ix) * INV_IH;
        // integrate velocities (gravity)
        hull.vy = hull.vy + GRAV * DT;
        leg[0].vy = leg[0].vy + GRAV * DT;
        leg[1].vy = leg[1].vy + GRAV * DT;
        // ---- contacts: initialise and warm-start
        float crx[8], cry[8], cnx[8], cny[8], cx0[8], ch0[8], cnm[8], ctm[8];
        bool con[8];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float sb, cb;
            sincos32(leg[b].ang, sb, cb);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = 4 * b + k;
                const float cx = (k == 1 || k == 2) ? LEG_HX : -LEG_HX, cy = k >= 2 ? LEG_HY : -LEG_HY;
                crx[q] = cb * cx - sb * cy;
                cry[q] = sb * cx + cb * cy;
                const float wx = leg[b].x + crx[q], wy = leg[b].y + cry[q];
                float dh;
                segment(wx, cx0[q], ch0[q], dh);
                const float ln = sqrtf(dh * dh + 4.0f);
                cnx[q] = -dh / ln;
                cny[q] = 2.0f / ln;
                const float sep = ((wx - cx0[q]) * cnx[q] + (wy - ch0[q]) * cny[q]) - RADIUS;
                con[q] = sep < 0.0f;
                can[q] = con[q] ? can[q] : 0.0f;
                cat[q] = con[q] ? cat[q] : 0.0f;
                const float tx = cny[q], ty = -cnx[q];
                const float rn = crx[q] * cny[q] - cry[q] * cnx[q];
                const float rt = crx[q] * ty - cry[q] * tx;
                cnm[q] = 1.0f / (INV_ML + INV_IL * (rn * rn));
                ctm[q] = 1.0f / (INV_ML + INV_IL * (rt * rt));
                if (con[q]) {
                    const float Px = can[q] * cnx[q] + cat[q] * tx, Py = can[q] * cny[q] + cat[q] * ty;
                    leg[b].vx = leg[b].vx + INV_ML * Px;
                    leg[b].vy = leg[b].vy + INV_ML * Py;
                    leg[b].om = leg[b].om + INV_IL * (crx[q] * Py - cry[q] * Px);
                }
            }
        }
        // ---- joints: initialise and warm-start
        const float rAx = -lx, rAy = -ly;
        float rBx[2], rBy[2], k11[2], k12[2], k22[2], idet[2], jang[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float sb, cb;
            sincos32(leg[b].ang, sb, cb);
            const float ax = (b == 0 ? -1.0f : 1.0f) * ANCX;
            rBx[b] = cb * ax - sb * ANCY;
            rBy[b] = sb * ax + cb * ANCY;
            k11[b] = ((INV_MH + INV_ML) + (rAy * rAy) * INV_IH) + (rBy[b] * rBy[b]) * INV_IL;
            k12[b] = (-(rAy * rAx) * INV_IH) - (rBy[b] * rBx[b]) * INV_IL;
            k22[b] = ((INV_MH + INV_ML) + (rAx * rAx) * INV_IH) + (rBx[b] * rBx[b]) * INV_IL;
            const float det = k11[b] * k22[b] - k12[b] * k12[b];
            idet[b] = det != 0.0f ? 1.0f / det : det;
            jang[b] = leg[b].ang - hull.ang;
            const float axial = (jm[b] + jlo[b]) - jup[b];
            hull.vx = hull.vx - INV_MH * jpx[b];
            hull.vy = hull.vy - INV_MH * jpy[b];
            hull.om = hull.om - INV_IH * ((rAx * jpy[b] - rAy * jpx[b]) + axial);
            leg[b].vx = leg[b].vx + INV_ML * jpx[b];
            leg[b].vy = leg[b].vy + INV_ML * jpy[b];
            leg[b].om = leg[b].om + INV_IL * ((rBx[b] * jpy[b] - rBy[b] * jpx[b]) + axial);
        }
        // ---- velocity sweeps: joints, then contacts
        for (int it = 0; it < vit; ++it) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float sg = b == 0 ? -1.0f : 1.0f, lo = b == 0 ? 0.4f : -0.9f, up = b == 0 ? 0.9f : -0.4f;
                // motor
                float cdot = (leg[b].om - hull.om) - sg * MOTOR_SPEED;
                float imp = -AXM * cdot;
                const float old = jm[b];
                jm[b] = clampf(old + imp, -MAX_MOTOR_IMP, MAX_MOTOR_IMP);
                imp = jm[b] - old;
                hull.om = hull.om - INV_IH * imp;
                leg[b].om = leg[b].om + INV_IL * imp;
                // lower limit
                float C = jang[b] - lo;
                cdot = leg[b].om - hull.om;
                imp = -AXM * (cdot + fmaxf(C, 0.0f) * INV_DT);
                float nw = fmaxf(jlo[b] + imp, 0.0f);
                imp = nw - jlo[b];
                jlo[b] = nw;
                hull.om = hull.om - INV_IH * imp;
                leg[b].om = leg[b].om + INV_IL * imp;
                // upper limit
                C = up - jang[b];
                cdot = hull.om - leg[b].om;
                imp = -AXM * (cdot + fmaxf(C, 0.0f) * INV_DT);
                nw = fmaxf(jup[b] + imp, 0.0f);
                imp = nw - jup[b];
                jup[b] = nw;
                hull.om = hull.om + INV_IH * imp;
                leg[b].om = leg[b].om - INV_IL * imp;
                // point
                const float cdx = ((leg[b].vx - leg[b].om * rBy[b]) - hull.vx) + hull.om * rAy;
                const float cdy = ((leg[b].vy + leg[b].om * rBx[b]) - hull.vy) - hull.om * rAx;
                const float bx = -cdx, by = -cdy;
                const float jx = idet[b] * (k22[b] * bx - k12[b] * by);
                const float jy = idet[b] * (k11[b] * by - k12[b] * bx);
                jpx[b] = jpx[b] + jx;
                jpy[b] = jpy[b] + jy;
                hull.vx = hull.vx - INV_MH * jx;
                hull.vy = hull.vy - INV_MH * jy;
                hull.om = hull.om - INV_IH * (rAx * jy - rAy * jx);
                leg[b].vx = leg[b].vx + INV_ML * jx;
                leg[b].vy = leg[b].vy + INV_ML * jy;
                leg[b].om = leg[b].om + INV_IL * (rBx[b] * jy - rBy[b] * jx);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int b = q >> 2;
                if (con[q]) {
                    const float tx = cny[q], ty = -cnx[q];
                    // tangent
                    float dvx = leg[b].vx - leg[b].om * cry[q];
                    float dvy = leg[b].vy + leg[b].om * crx[q];
                    float lam = ctm[q] * -(dvx * tx + dvy * ty);
                    const float lim = MU3 * can[q];
                    float nw = clampf(cat[q] + lam, -lim, lim);
                    lam = nw - cat[q];
                    cat[q] = nw;
                    float Px = lam * tx, Py = lam * ty;
                    leg[b].vx = leg[b].vx + INV_ML * Px;
                    leg[b].vy = leg[b].vy + INV_ML * Py;
                    leg[b].om = leg[b].om + INV_IL * (crx[q] * Py - cry[q] * Px);
                    // normal
                    dvx = leg[b].vx - leg[b].om * cry[q];
                    dvy = leg[b].vy + leg[b].om * crx[q];
                    lam = -cnm[q] * (dvx * cnx[q] + dvy * cny[q]);
                    nw = fmaxf(can[q] + lam, 0.0f);
                    lam = nw - can[q];
                    can[q] = nw;
                    Px = lam * cnx[q]; Py = lam * cny[q];
                    leg[b].vx = leg[b].vx + INV_ML * Px;
                    leg[b].vy = leg[b].vy + INV_ML * Py;
                    leg[b].om = leg[b].om + INV_IL * (crx[q] * Py - cry[q] * Px);
                }
            }
        }
        // ---- integrate positions
        hull.x = hull.x + DT * hull.vx; hull.y = hull.y + DT * hull.vy; hull.ang = hull.ang + DT * hull.om;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            leg[b].x = leg[b].x + DT * leg[b].vx; leg[b].y = leg[b].y + DT * leg[b].vy; leg[b].ang = leg[b].ang + DT * leg[b].om;
        }
        // ---- position sweeps: contacts, then joints; a solved env leaves the loop (Box2D's per-island early exit: a per-lane branch)
        bool solved = false;
        for (int it = 0; it < pit && !solved; ++it) {
            float minsep = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int b = q >> 2, k = q & 3;
                if (con[q]) {
                    const float cx = (k == 1 || k == 2) ? LEG_HX : -LEG_HX, cy = k >= 2 ? LEG_HY : -LEG_HY;
                    float sb, cb;
                    sincos32(leg[b].ang, sb, cb);
                    const float qx = cb * cx - sb * cy, qy = sb * cx + cb * cy;
                    const float wx = leg[b].x + qx, wy = leg[b].y + qy;
                    const float sep = ((wx - cx0[q]) * cnx[q] + (wy - ch0[q]) * cny[q]) - RADIUS;
                    minsep = fminf(minsep, sep);
                    const float C = clampf(BAUM * (sep + SLOP), -MAXLC, 0.0f);
                    const float rn = qx * cny[q] - qy * cnx[q];
                    const float K = INV_ML + INV_IL * (rn * rn);
                    const float imp = -C / K;
                    const float Px = imp * cnx[q], Py = imp * cny[q];
                    leg[b].x = leg[b].x + INV_ML * Px;
                    leg[b].y = leg[b].y + INV_ML * Py;
                    leg[b].ang = leg[b].ang + INV_IL * (qx * Py - qy * Px);
                }
            }
            bool jok = true;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float sg = b == 0 ? -1.0f : 1.0f, lo = b == 0 ? 0.4f : -0.9f, up = b == 0 ? 0.9f : -0.4f;
                const float angle = leg[b].ang - hull.ang;
                const float C = angle <= lo ? clampf((angle - lo) + ASLOP, -MAXAC, 0.0f)
                                            : (angle >= up ? clampf((angle - up) - ASLOP, 0.0f, MAXAC) : 0.0f);
                const float limp = -AXM * C;
                float hang = hull.ang - INV_IH * limp;
                float lang = leg[b].ang + INV_IL * limp;
                float sa, ca, sb, cb;
                sincos32(hang, sa, ca);
                sincos32(lang, sb, cb);
                const float pAx = sa * LCY, pAy = -(ca * LCY);
                const float ax = sg * ANCX;
                const float pBx = cb * ax - sb * ANCY, pBy = sb * ax + cb * ANCY;
                const float Cx = ((leg[b].x + pBx) - hull.x) - pAx;
                const float Cy = ((leg[b].y + pBy) - hull.y) - pAy;
                const float perr = sqrtf(Cx * Cx + Cy * Cy);
                const float a11 = ((INV_MH + INV_ML) + (pAy * pAy) * INV_IH) + (pBy * pBy) * INV_IL;
                const float a12 = (-(pAy * pAx) * INV_IH) - (pBy * pBx) * INV_IL;
                const float a22 = ((INV_MH + INV_ML) + (pAx * pAx) * INV_IH) + (pBx * pBx) * INV_IL;
                const float det = a11 * a22 - a12 * a12;
                const float id = det != 0.0f ? 1.0f / det : det;
                const float jx = -(id * (a22 * Cx - a12 * Cy));
                const float jy = -(id * (a11 * Cy - a12 * Cx));
                hull.x = hull.x - INV_MH * jx;
                hull.y = hull.y - INV_MH * jy;
                hang = hang - INV_IH * (pAx * jy - pAy * jx);
                leg[b].x = leg[b].x + INV_ML * jx;
                leg[b].y = leg[b].y + INV_ML * jy;
                lang = lang + INV_IL * (pBx * jy - pBy * jx);
                hull.ang = hang;
                leg[b].ang = lang;
                jok = jok && (perr <= SLOP) && (fabsf(C) <= ASLOP);
            }
            solved = (minsep >= SLOP3N) && jok;
        }
        // ---- the step's flags, the hull origin at the new pose, crash test on the hull vertices
        c1 = (con[0] || con[1] || con[2] || con[3]) ? 1.0f : 0.0f;
        c2 = (con[4] || con[5] || con[6] || con[7]) ? 1.0f : 0.0f;
        pstep = pstep + 1.0f;
        sincos32(hull.ang, sn, cs);
        px = hull.x + sn * LCY;
        py = hull.y - cs * LCY;
        bool crash = false;
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            const float hx = HULLX[v], hy = HULLY[v];
            const float wx = px + (cs * hx - sn * hy);
            const float wy = py + (sn * hx + cs * hy);
            crash = crash || (wy < ground(wx));
        }
        // rest detection (b2Island::Solve's sleep test)
        bool slow = ((hull.vx * hull.vx + hull.vy * hull.vy) <= SLEEP_LIN2) && ((hull.om * hull.om) <= SLEEP_ANG2);
#pragma unroll
        for (int b = 0; b < 2; ++b)
            slow = slow && ((leg[b].vx * leg[b].vx + leg[b].vy * leg[b].vy) <= SLEEP_LIN2) && ((leg[b].om * leg[b].om) <= SLEEP_ANG2);
        sleep = slow ? sleep + 1.0f : 0.0f;
        const bool asleep = (sleep >= SLEEP_STEPS) && solved;
        obs(o);
        const float shaping = ((-100.0f * sqrtf(o[0] * o[0] + o[1] * o[1]) - 100.0f * sqrtf(o[2] * o[2] + o[3] * o[3])) -
                               100.0f * fabsf(o[4])) + 10.0f * o[6] + 10.0f * o[7];
        float rew = hasp > 0.0f ? shaping - prev : 0.0f;
        prev = shaping;
        hasp = 1.0f;
        rew = (rew - m_power * 0.30f) - s_power * 0.03f;
        const bool out = crash || (fabsf(o[0]) >= 1.0f);
        rew = out ? -100.0f : (asleep ? 100.0f : rew);
        done_env = out || asleep;
        return rew;
    }
    // env.reset(): terrain, the three bodies, random initial force, one no-op step (oracle: Lander3Oracle.reset)
    __device__ void reset(float *o) {
        float hs[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) hs[j] = rng(RESET_STREAM, j) * 6.6666665f;
#pragma unroll
        for (int j = 3; j < 8; ++j) hs[j] = HELIPAD_Y;
#pragma unroll
        for (int i = 0; i < 11; ++i) terr[i] = 0.33f * ((hs[(i + 11) % 12] + hs[i]) + hs[i + 1]);
        const float fx = (rng(RESET_STREAM, 12) * 2.0f - 1.0f) * 1000.0f;
        const float fy = (rng(RESET_STREAM, 13) * 2.0f - 1.0f) * 1000.0f;
        hull.x = 10.0f; hull.y = H_ + LCY; hull.ang = 0.0f;
        px = 10.0f; py = H_;
        hull.vx = (fx * DT) * INV_MH; hull.vy = (fy * DT) * INV_MH; hull.om = 0.0f;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float sg = b == 0 ? -1.0f : 1.0f;
            leg[b].x = 10.0f - sg * LEG_X0; leg[b].y = H_; leg[b].ang = sg * LEG_A0;
            leg[b].vx = leg[b].vy = leg[b].om = 0.0f;
            jpx[b] = jpy[b] = jm[b] = jlo[b] = jup[b] = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) can[q] = cat[q] = 0.0f;
        c1 = c2 = prev = hasp = eplen = epret = sleep = pstep = 0.0f;
        bool d;
        (void)physics(0.0f, 0.0f, d, o);
    }
    __device__ void load(const float *S, long long n, long long i) {
        hull.x = S[X * n + i]; hull.y = S[Y * n + i]; hull.vx = S[VX * n + i]; hull.vy = S[VY * n + i]; hull.ang = S[ANG * n + i];
        hull.om = S[OM * n + i]; c1 = S[C1 * n + i]; c2 = S[C2 * n + i]; prev = S[PREV * n + i]; hasp = S[HASP * n + i];
        eplen = S[EPLEN * n + i]; epret = S[EPRET * n + i]; sleep = S[SLEEP * n + i]; epi = S[EPI * n + i];
        pstep = S[PSTEP * n + i]; px = S[PX * n + i]; py = S[PY * n + i];
#pragma unroll
        for (int t = 0; t < 11; ++t) terr[t] = S[(T0 + t) * n + i];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float *L = S + (long long)(L0 + 6 * b) * n + i;
            leg[b].x = L[0]; leg[b].y = L[n]; leg[b].vx = L[2 * n]; leg[b].vy = L[3 * n]; leg[b].ang = L[4 * n]; leg[b].om = L[5 * n];
            const float *J = S + (long long)(J0 + 5 * b) * n + i;
            jpx[b] = J[0]; jpy[b] = J[n]; jm[b] = J[2 * n]; jlo[b] = J[3 * n]; jup[b] = J[4 * n];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            can[q] = S[(long long)(K0 + 2 * q) * n + i];
            cat[q] = S[(long long)(K0 + 2 * q + 1) * n + i];
        }
    }
    __device__ void store(float *S, long long n, long long i) const {
        S[X * n + i] = hull.x; S[Y * n + i] = hull.y; S[VX * n + i] = hull.vx; S[VY * n + i] = hull.vy; S[ANG * n + i] = hull.ang;
        S[OM * n + i] = hull.om; S[C1 * n + i] = c1; S[C2 * n + i] = c2; S[PREV * n + i] = prev; S[HASP * n + i] = hasp;
        S[EPLEN * n + i] = eplen; S[EPRET * n + i] = epret; S[SLEEP * n + i] = sleep; S[EPI * n + i] = epi;
        S[PSTEP * n + i] = pstep; S[PX * n + i] = px; S[PY * n + i] = py;
#pragma unroll
        for (int t = 0; t < 11; ++t) S[(T0 + t) * n + i] = terr[t];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float *L = S + (long long)(L0 + 6 * b) * n + i;
            L[0] = leg[b].x; L[n] = leg[b].y; L[2 * n] = leg[b].vx; L[3 * n] = leg[b].vy; L[4 * n] = leg[b].ang; L[5 * n] = leg[b].om;
            float *J = S + (long long)(J0 + 5 * b) * n + i;
            J[0] = jpx[b]; J[n] = jpy[b]; J[2 * n] = jm[b]; J[3 * n] = jlo[b]; J[4 * n] = jup[b];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            S[(long long)(K0 + 2 * q) * n + i] = can[q];
            S[(long long)(K0 + 2 * q + 1) * n + i] = cat[q];
        }
    }
};

}  // namespace
