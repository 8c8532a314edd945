// tests/native/check_skywin.cpp -- the v4 kernels' sky window (csrc/pt_v4_skywin.h: one slope rectangle
// per object for a (scene, camera); a camera ray outside every rectangle skips TestSceneTrace) against
// the v4 oracle's TestSceneTrace (oracle/pt_oracle_v4.c pto4_trace_scene, the reference's f32
// operations).  The header is compiled for the host: the window builder and the very predicate the
// kernels run.
//
// Scenes: the test scene of tests/v4_camera_oracle.py, InitializeScene, three seeded random scenes
// (non-planar quads, spheres down to radius 0.01).  Cameras: the default one and A, B, C of
// tests/v4_camera_oracle.py.  Rays per (scene, camera): slope grids across every edge of every
// rectangle (one over +-3 margins, two over +-2e-3 and +-2e-4 of slope around the unwidened edge)
// and every camera ray of a 256 x 144 image with the jitter at its four extremes.
//   1. no ray the predicate classifies as sky may hit;
//   2. for every ray that hits, the slope distance of the ray outside the UNWIDENED rectangle of the
//      object it hit is measured: the largest one is the "observed outside-hit distance", and the
//      margin of that rectangle side must be at least 100 times it (a pin-point sphere's discriminant
//      rounding inflates it visibly, and its sides carry their own, larger margin: reported apart;
//      the smallest margin of any side must also be 100 times the distance observed on all other
//      objects).
// usage: check_skywin    exit 0 iff both hold
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../cpuperformanceraytracer_amd/csrc/pt_v4_skywin.h"
#include "../../oracle/pt_oracle.h"

namespace {

struct Camera {
    const char* name;
    float pos[3], fov;
};
const Camera kCameras[] = {{"default", {0.0f, 0.0f, 40.0f}, 90.0f},
                           {"A", {3.0f, -2.0f, 30.0f}, 60.0f},
                           {"B", {-6.5f, 4.25f, 55.0f}, 90.0f},
                           {"C", {0.0f, -6.0f, 22.0f}, 75.0f}};

float camera_distance(float fov) { return 1.0f / tanf(fov * 0.5f * 3.14159265359f / 180.0f); }   // v4 :1500

void normalize_fma(float v[3])   // v4's normalize: v * (1 / sqrt(dot)), dot = fma(x,x', fma(y,y', z*z'))
{
    const float inv = 1.0f / std::sqrt(std::fmaf(v[0], v[0], std::fmaf(v[1], v[1], v[2] * v[2])));
    v[0] *= inv, v[1] *= inv, v[2] *= inv;
}

void quad(pto4_scene& s, const float v[4][3]) { std::memcpy(s.quad[s.nquads++], v, 12 * sizeof(float)); }
void sphere(pto4_scene& s, float x, float y, float z, float r)
{
    const float p[4] = {x, y, z, r};
    std::memcpy(s.sphere[s.nspheres++], p, sizeof(p));
}

void test_scene(pto4_scene& s)   // tests/v4_camera_oracle.py QUADS / SPHERES
{
    std::memset(&s, 0, sizeof(s));
    const float floor_[4][3] = {{-10, -8, 2}, {10, -8, 2}, {10, -8, 16}, {-10, -8, 16}};
    const float light[4][3] = {{-4, 6, 6}, {4, 6, 6}, {4, 6, 12}, {-4, 6, 12}};
    quad(s, floor_);
    quad(s, light);
    sphere(s, -4.0f, -5.0f, 9.0f, 3.0f);
    sphere(s, 5.0f, -4.5f, 11.0f, 3.5f);
    s.nmat = s.nquads + s.nspheres;
}

uint32_t g_rng;
float rnd(float lo, float hi)   // (an LCG: the same scenes on every run)
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(g_rng >> 8) * (1.0f / 16777216.0f);
}
void random_scene(pto4_scene& s, uint32_t seed)   // everything at z <= 20.5: >= 1.5 in front of camera C
{
    std::memset(&s, 0, sizeof(s));
    g_rng = seed;
    const int nq = 1 + (int)rnd(0.0f, 4.99f), ns = 1 + (int)rnd(0.0f, 4.99f);
    for (int i = 0; i < nq; ++i) {
        // a rough rectangle around a centre, every vertex displaced on its own: not planar
        const float c[3] = {rnd(-12, 12), rnd(-10, 10), rnd(-8, 14)};
        const float e[2] = {rnd(0.5f, 8), rnd(0.5f, 8)};
        const int ax = (int)rnd(0.0f, 2.99f);   // the axis the rectangle is (roughly) normal to
        float v[4][3];
        for (int k = 0; k < 4; ++k) {
            const float a = (k == 1 || k == 2) ? e[0] : -e[0], b = k >= 2 ? e[1] : -e[1];
            const float off[3][3] = {{0, a, b}, {a, 0, b}, {a, b, 0}};
            for (int j = 0; j < 3; ++j) v[k][j] = c[j] + off[ax][j] + rnd(-0.4f, 0.4f);
            if (v[k][2] > 20.5f) v[k][2] = 20.5f;
        }
        quad(s, v);
    }
    for (int i = 0; i < ns; ++i) {
        const float r = i == 0 ? 0.01f : rnd(0.3f, 3.0f);   // the first one a pin-point (the margin's worst case)
        sphere(s, rnd(-12, 12), rnd(-10, 10), rnd(-8, 20.5f - r), r);
    }
    s.nmat = s.nquads + s.nspheres;
}

long long n_rays = 0, n_sky = 0, n_hit = 0, n_bad = 0;
double max_out = 0.0, max_out_pin = 0.0, max_ratio = 0.0, min_margin = INFINITY;   // (pin: spheres of radius < 0.1)

struct Case {
    const pto4_scene* scene;
    const float* P;
    PtV4SkyWin wide, tight;   // the kernels' window; the unwidened rectangles
};

void check(const Case& c, const float D[3])
{
    ++n_rays;
    int mat = -1;
    const bool hit = pto4_trace_scene(c.scene, c.P, D, &mat) != 10000.0f;
    const bool sky = pt_v4_skywin_sky(c.wide, D[0], D[1], D[2]);
    n_sky += sky;
    n_hit += hit;
    if (sky && hit && ++n_bad <= 20)
        std::printf("SKY RAY HITS object %d  P=(%g, %g, %g) D=(%a, %a, %a)\n", mat, c.P[0], c.P[1], c.P[2], D[0], D[1], D[2]);
    if (hit && mat >= 0 && mat < c.tight.nrects && D[2] < 0.0f) {
        const double s[2] = {(double)D[0] / -(double)D[2], (double)D[1] / -(double)D[2]};
        const float *t = c.tight.rect[mat], *w = c.wide.rect[mat];
        const bool pin = mat >= c.scene->nquads && c.scene->sphere[mat - c.scene->nquads][3] < 0.1f;
        double& worst = pin ? max_out_pin : max_out;
        for (int a = 0; a < 2; ++a) {
            const double out_lo = (double)t[2 * a] - s[a], out_hi = s[a] - (double)t[2 * a + 1];
            if (out_lo > 0.0) {
                worst = std::fmax(worst, out_lo);
                max_ratio = std::fmax(max_ratio, out_lo / ((double)t[2 * a] - (double)w[2 * a]));
            }
            if (out_hi > 0.0) {
                worst = std::fmax(worst, out_hi);
                max_ratio = std::fmax(max_ratio, out_hi / ((double)w[2 * a + 1] - (double)t[2 * a + 1]));
            }
        }
    }
}

void slope_ray(const Case& c, double sx, double sy)
{
    float D[3] = {(float)sx, (float)sy, -1.0f};
    normalize_fma(D);
    check(c, D);
}

// grids across the four edges of rectangle i: n1 steps across the edge over +-half, n2 along it
void edge_grids(const Case& c, int i, double half_scale, double half_abs, int n1, int n2)
{
    const float *t = c.tight.rect[i], *w = c.wide.rect[i];
    for (int a = 0; a < 2; ++a)         // the axis the edge bounds
        for (int side = 0; side < 2; ++side) {
            const double edge = t[2 * a + side];
            const double half = half_abs + half_scale * std::fabs((double)w[2 * a + side] - edge);
            // (along the edge: the unwidened extent and a little more -- a small object is not stepped over)
            const double lo = t[2 * (1 - a)], hi = t[2 * (1 - a) + 1], pad = 0.1 * (hi - lo) + 5e-4;
            for (int p = 0; p < n1; ++p)
                for (int q = 0; q < n2; ++q) {
                    const double u = edge - half + 2.0 * half * (p + 0.5) / n1;
                    const double v = lo - pad + (hi - lo + 2.0 * pad) * (q + 0.5) / n2;
                    if (a == 0) slope_ray(c, u, v);
                    else slope_ray(c, v, u);
                }
        }
}

void image(const Case& c, float dist, int w, int h)   // mainImage v4 :1092-1113, the jitter at its extremes
{
    const float rW = 1.0f / (float)w, rH = 1.0f / (float)h, H = (float)h;
    const float jit[2] = {-0.5f, 0.49999997f};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int jx = 0; jx < 2; ++jx)
                for (int jy = 0; jy < 2; ++jy) {
                    const float tx = std::fmaf(((float)x + jit[jx]) * rW, 2.0f, -1.0f);
                    float ty = std::fmaf(((float)(h - 1 - y) + jit[jy]) * rH, 2.0f, -1.0f);
                    ty = ty * (rW * H);
                    float D[3] = {tx, ty, -dist};
                    normalize_fma(D);
                    check(c, D);
                }
}

}  // namespace

int main()
{
    pto4_scene scenes[5];
    test_scene(scenes[0]);
    pto4_default_scene(&scenes[1]);
    for (int k = 0; k < 3; ++k) random_scene(scenes[2 + k], 1234u + 77u * (uint32_t)k);
    int n_windows = 0;
    for (const pto4_scene& s : scenes)
        for (const Camera& cam : kCameras) {
            Case c{&s, cam.pos, {}, {}};
            const int n = pt_v4_skywin_build(s.nquads, s.quad, s.nspheres, s.sphere, cam.pos, &c.wide);
            pt_v4_skywin_build(s.nquads, s.quad, s.nspheres, s.sphere, cam.pos, &c.tight, 0.0);
            if (n != s.nquads + s.nspheres || c.tight.nrects != n) {
                std::printf("NO WINDOW for a scene in front of camera %s (nrects %d)\n", cam.name, n);
                return 2;
            }
            ++n_windows;
            for (int i = 0; i < n; ++i) {
                for (int k = 0; k < 4; ++k)
                    min_margin = std::fmin(min_margin, std::fabs((double)c.wide.rect[i][k] - (double)c.tight.rect[i][k]));
                edge_grids(c, i, 3.0, 0.0, 64, 64);     // +-3 margins across each edge
                edge_grids(c, i, 0.0, 2e-3, 64, 48);    // +-2e-3 of slope around the unwidened edge
                edge_grids(c, i, 0.0, 2e-4, 33, 64);    // +-2e-4
            }
            image(c, camera_distance(cam.fov), 256, 144);
        }
    // a camera inside the scene's depth range has no window
    {
        const float P[3] = {0.0f, 0.0f, 8.0f};
        PtV4SkyWin w;
        if (pt_v4_skywin_build(scenes[0].nquads, scenes[0].quad, scenes[0].nspheres, scenes[0].sphere, P, &w) != -1 ||
            pt_v4_skywin_sky(w, 0.0f, 0.9f, -0.1f)) {
            std::printf("a window exists for a camera inside the scene\n");
            return 2;
        }
    }
    std::printf("windows %d  rays %lld  hits %lld  classified sky %lld  sky rays that hit %lld\n", n_windows, n_rays, n_hit,
                n_sky, n_bad);
    // (the margin is per rectangle side: a pin-point sphere's is larger, pt_v4_skywin.h)
    std::printf("observed outside-hit distance %.3e (pin-point spheres %.3e)  smallest margin %.3e  largest distance/margin %.3e\n",
                max_out, max_out_pin, min_margin, max_ratio);
    return n_bad || !(max_ratio <= 0.01) || !(min_margin >= 100.0 * max_out) ? 1 : 0;
}
