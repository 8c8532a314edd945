// pt_v4_skywin.h -- the v4 kernels' sky test for an arbitrary (scene, camera): the sky window.
// Shared by the host (pt_capi.cpp builds the window; tests/native/check_skywin.cpp checks it against
// the v4 oracle's TestSceneTrace) and the kernels (pt_v4.hip consults it), like pt_quadcull.h.
//
// What.  The v4 camera looks down -z with no roll (mainImage v4 :1092-1130), so a camera ray from P
// with direction D (D.z < 0) is described by its slopes sx = D.x / -D.z, sy = D.y / -D.z: the point
// P + t D at depth t -D.z in front of the camera lies at lateral offset (sx, sy) x depth.  For every
// object the host computes one slope rectangle [sx_lo, sx_hi] x [sy_lo, sy_hi] that contains the
// slopes of all its points; a ray whose slopes lie outside every rectangle passes no object and is
// the reference's miss ("sky").  Where the default scene's instances consult sky_ray_v4, the generic
// instances consult the window: when every busy lane of a wave traces a sky camera ray the wave takes
// TestSceneTrace's miss (v4 :700-718: dist = c_superFar) without running the tests.
//
// Rectangles (evaluated in double from the f32 scene description and camera position):
//   quad    the bounding box of the projections (v - P).xy / (P.z - v.z) of its four vertices and of
//           two more points, Q2 and Q3.  TestQuadTrace (:556-637) intersects the ray with the plane of
//           triangle (V0, V1, V2) (n and V0, PrecomputeQuadData :269-320) and tests the hit point hp
//           (relative to V0) in two triangles.  The first, B = (dot(hp, n x V01), dot(hp, n x V20)) /
//           DetBot, is triangle (V0, V1, V2) itself.  The second is B0 = dot(hp, n x V30) / DetTop, B1 =
//           dot(hp, n x V02) / DetTop, B2 = 1 - B0 - B1 >= 0.  Neither dot changes when V3 moves along
//           n, so it sees V3' = V3 moved into the plane; and DetTop is n . (V30 x V01) (:283), which
//           equals the triangle's own determinant n . (V02 x V03) only for a parallelogram.  With rho
//           = n . (V02 x V03) / DetTop, (B0, B1) are rho times the barycentrics of (V2, V3') in triangle
//           (V0, V2, V3'): the accepted region is that triangle scaled about V0 by 1 / rho (mirrored
//           when rho < 0), corners V0, Q2 = V0 + V02 / rho, Q3 = V0 + (V3' - V0) / rho.  For a planar
//           parallelogram -- every quad of InitializeScene -- Q2 = V2 and Q3 = V3; for any other quad the
//           bounding box of the four vertices alone misses part of what the reference hits
//           (check_skywin.cpp's random scenes found it).  The regions are convex hulls of these points,
//           the projection maps segments in front of the camera to segments, and a box is convex:
//           every accepted point projects inside it.  A quad with a sliver triangle (|a x b| < 1e-3
//           |a| |b| for its edge pairs: rho and n carry no accuracy in f32) has no window.
//   sphere  max over the ball of x / depth is the max over the ball's projection onto the (x, depth)
//           plane, the disc of radius r around (c.x - P.x, P.z - c.z): the slopes of its two tangents
//           from the origin, tan(phi -+ alpha), phi = atan2(offset, depth), alpha = asin(r / rho).
//           The same in (y, depth).
// The window exists only when every coordinate (vertices, centres, radii, camera) is finite and within
// +-1024, no radius is negative, and every vertex (Q2, Q3 included) and every sphere's nearest point
// (P.z - c.z - r) is at least 1.0 in front of the camera -- otherwise nrects = -1 and nothing is skipped.  (An empty scene
// has the empty window, nrects = 0: every camera ray is sky.)
//
// Margin.  The reference decides a hit in f32, so its silhouettes differ from the exact ones by its
// rounding, eps = 2^-24 per operation, on operands no larger than R = the largest |coordinate of
// (vertex or centre) - P| + r of the object:
//   TestQuadTrace   off = v0 - pos (eps R per component), dist = dot(off, n) / dot(dir, n) (two fused
//       3-term dots and a division), hp = dist dir - off (eps (|dist| + R) <= 3 eps R per component), then
//       six dots of hp with the precomputed edge vectors NxV / Det (:269-320, themselves ~8 eps
//       relative), compared with 0 and 1.  An error of dist moves hp along the ray: the in-plane
//       shift it causes corresponds to a change of the ray by that shift x |dot(dir, n)| / dist, which
//       cancels the 1 / dot(dir, n) growth of dist's error at grazing incidence.  In all the accepted
//       region is the exact one moved by <= ~20 eps R in space (1e-6 R).
//   TestSphereTrace  m = pos - c, b = dot(m, dir), cc = dot(m, m) - r r, discr = b b - cc >= 0: the
//       accepted lines are those within sqrt(r r + e) of the centre, |e| <= ~8 eps |m|^2 the rounding
//       of discr (b b and dot(m, m) are both ~|m|^2 and cancel).  For an ordinary sphere that is a
//       growth of e / 2r (1e-4 at r = 3, |m| = 40); for a pin-point one (r -> 0) it is sqrt(8 eps) |m|
//       = 7e-4 |m|, larger than the sphere -- the one rounding effect that is not ~eps R.
// A displacement delta of a silhouette point at depth >= d_min changes its slope by <= delta (1 + |s|) /
// d_min: ~1e-6 (1 + |s|) R / d_min for quads and centres.  Every side of a rectangle (s its own slope)
// is widened by
//     margin = (1 + |s|) x (kPtSkyWinMargin x max(1, R / d_min) + kPtSkyWinGrow x grow / d_min)
//     kPtSkyWinMargin = 2^-8 (3.9e-3),  kPtSkyWinGrow = 256,  grow = sqrt(r r + 8 eps |m|^2) - r (spheres)
// i.e. >= 1000 times the ~eps R bound, and 256 times a sphere's own growth bound on top -- far above
// the kernel's rounding of the comparison D.x < lo x -D.z (eps |s|) and of the window's conversion
// to f32 (rounded outwards anyway).  tests/native/check_skywin.cpp measures the largest slope distance
// outside the UNWIDENED rectangles at which the oracle still reports a hit, and requires every such
// hit to lie within 1 % of its side's margin (DESIGN.md 3b records the figures: 4.6e-8 on ordinary
// objects against a smallest margin of 3.96e-3; 4.3e-4 on spheres of radius 0.01, about 0.7 of their
// growth bound; the largest observed / margin ratio of any side 2.7e-3).  For InitializeScene seen from (0, 0, 40) the margin is
// 0.004-0.01 of slope (R / d_min <= 1.8), 4-10 pixels at 1080p -- the default camera's own instances
// keep sky_ray_v4's hand-derived thresholds.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_SKYWIN_HD __host__ __device__ __forceinline__
#else
#define PT_SKYWIN_HD inline
#endif

#define PT_V4_SKYWIN_MAX 12   // PT_V4_MAX_OBJECTS (pt_v4.h asserts)

constexpr double kPtSkyWinMargin = 0x1p-8;
constexpr double kPtSkyWinDiscrEps = 8.0 * 0x1p-24;   // TestSphereTrace's discriminant: <= 8 eps |m|^2 of rounding
constexpr double kPtSkyWinGrow = 256.0;               // the margin's multiple of a sphere's radius inflation
constexpr double kPtSkyWinMinDepth = 1.0;   // every object at least this far in front of the camera
constexpr double kPtSkyWinMaxCoord = 1024.0;
constexpr double kPtSkyWinMinSine = 1e-3;    // a quad's triangles: |a x b| >= this x |a| |b|

// One rectangle per object, quads first (the scene's object order): sx_lo, sx_hi, sy_lo, sy_hi.
struct PtV4SkyWin {
    int32_t nrects;   // -1: no window, nothing is skipped
    float rect[PT_V4_SKYWIN_MAX][4];
};

// A camera ray (direction D, any length) that lies outside every rectangle of the window.  False
// without a window, for D.z >= 0 and for a NaN direction.
PT_SKYWIN_HD bool pt_v4_skywin_sky(const PtV4SkyWin& w, float dx, float dy, float dz)
{
    const float nz = -dz;
    bool sky = w.nrects >= 0 && nz > 0.0f && dx == dx && dy == dy;
    for (int i = 0; i < w.nrects; ++i) {
        const float* r = w.rect[i];
        sky = sky && (dx < r[0] * nz || dx > r[1] * nz || dy < r[2] * nz || dy > r[3] * nz);
    }
    return sky;
}

// Host: the window of the scene description (quads' vertices, spheres' centre and radius, as passed to
// AddQuadObjectToScene / AddSphereObjectToScene) seen from P.  margin_scale 1: the margin above; 0:
// the unwidened rectangles (the checker's measurement).  Returns out->nrects.
inline int32_t pt_v4_skywin_build(int32_t nquads, const float (*quad)[4][3], int32_t nspheres, const float (*sphere)[4],
                                  const float P[3], PtV4SkyWin* out, double margin_scale = 1.0)
{
    PtV4SkyWin w{};
    w.nrects = -1;
    *out = w;
    if (nquads < 0 || nspheres < 0 || nquads + nspheres > PT_V4_SKYWIN_MAX) return -1;
    const auto ok = [](double v) { return isfinite(v) && fabs(v) <= kPtSkyWinMaxCoord; };
    for (int k = 0; k < 3; ++k)
        if (!ok((double)P[k])) return -1;
    int n = 0;
    // lo/hi of the object's slopes, R its largest offset from P, dmin its smallest depth
    // (grow: a sphere's radius inflation by the rounding of its discriminant, 0 for quads)
    const auto emit = [&](const double lo[2], const double hi[2], double R, double dmin, double grow) {
        const double g = margin_scale * (kPtSkyWinMargin * fmax(1.0, R / dmin) + kPtSkyWinGrow * grow / dmin);
        float* r = w.rect[n++];
        for (int a = 0; a < 2; ++a) {
            // (nextafter: the conversion to f32 never rounds a side inwards, also with margin_scale 0)
            r[2 * a] = nextafterf((float)(lo[a] - g * (1.0 + fabs(lo[a]))), -INFINITY);
            r[2 * a + 1] = nextafterf((float)(hi[a] + g * (1.0 + fabs(hi[a]))), INFINITY);
        }
    };
    for (int i = 0; i < nquads; ++i) {
        double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY}, R = 0.0, dmin = INFINITY;
        // the four vertices and the second triangle's accepted corners Q2, Q3 (the header comment)
        double pt[6][3];
        for (int v = 0; v < 4; ++v)
            for (int k = 0; k < 3; ++k) pt[v][k] = (double)quad[i][v][k];
        {
            const auto cross = [](const double a[3], const double b[3], double c[3]) {
                c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
            };
            const auto dot = [](const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
            double e1[3], e2[3], e3[3], n[3], c23[3], c31[3];
            for (int k = 0; k < 3; ++k) e1[k] = pt[1][k] - pt[0][k], e2[k] = pt[2][k] - pt[0][k], e3[k] = pt[3][k] - pt[0][k];
            cross(e1, e2, n);
            const double l1 = sqrt(dot(e1, e1)), l2 = sqrt(dot(e2, e2)), l3 = sqrt(dot(e3, e3)), ln = sqrt(dot(n, n));
            // (a sliver: the f32 normal and determinants carry no accuracy -- no window)
            if (!(ln >= kPtSkyWinMinSine * l1 * l2)) return -1;
            for (int k = 0; k < 3; ++k) n[k] /= ln;
            cross(e2, e3, c23);   // V02 x V03: twice the second triangle's area vector
            cross(e1, e3, c31);   // V30 x V01 (= V01 x V03), the reference's "V02xV03" (:283)
            const double det_true = dot(c23, n), det_ref = dot(c31, n);
            if (!(fabs(det_true) >= kPtSkyWinMinSine * l2 * l3 && fabs(det_ref) >= kPtSkyWinMinSine * l1 * l3)) return -1;
            const double inv_rho = det_ref / det_true, t = dot(e3, n);
            for (int k = 0; k < 3; ++k) {
                pt[4][k] = pt[0][k] + inv_rho * e2[k];
                pt[5][k] = pt[0][k] + inv_rho * (e3[k] - t * n[k]);
            }
        }
        for (int v = 0; v < 6; ++v) {
            const double* q = pt[v];
            if (!ok(q[0]) || !ok(q[1]) || !ok(q[2])) return -1;
            const double depth = (double)P[2] - (double)q[2];
            if (!(depth >= kPtSkyWinMinDepth)) return -1;
            dmin = fmin(dmin, depth);
            R = fmax(R, depth);
            for (int a = 0; a < 2; ++a) {
                const double off = (double)q[a] - (double)P[a];
                R = fmax(R, fabs(off));
                lo[a] = fmin(lo[a], off / depth);
                hi[a] = fmax(hi[a], off / depth);
            }
        }
        emit(lo, hi, R, dmin, 0.0);
    }
    for (int i = 0; i < nspheres; ++i) {
        const float* s = sphere[i];
        if (!ok((double)s[0]) || !ok((double)s[1]) || !ok((double)s[2]) || !ok((double)s[3]) || s[3] < 0.0f) return -1;
        const double r = (double)s[3], depth = (double)P[2] - (double)s[2];
        if (!(depth - r >= kPtSkyWinMinDepth)) return -1;
        double lo[2], hi[2], R = depth + r, m2 = depth * depth;
        for (int a = 0; a < 2; ++a) {
            const double off = (double)s[a] - (double)P[a];
            R = fmax(R, fabs(off) + r);
            m2 += off * off;
            // the disc of radius r around (off, depth), depth - r >= 1: both tangents lie in front
            const double phi = atan2(off, depth), alpha = asin(fmin(1.0, r / hypot(off, depth)));
            lo[a] = tan(phi - alpha);
            hi[a] = tan(phi + alpha);
        }
        // TestSphereTrace accepts discr = b b - (|m|^2 - r r) >= 0 computed in f32: an error of up to
        // kPtSkyWinDiscrEps |m|^2, i.e. the sphere of radius sqrt(r r + that) -- which matters when r is small
        emit(lo, hi, R, depth - r, sqrt(r * r + kPtSkyWinDiscrEps * m2) - r);
    }
    w.nrects = n;
    *out = w;
    return n;
}
