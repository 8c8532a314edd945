// oracle/ref_v4.cpp -- TEST INFRASTRUCTURE ONLY (our code, no reference text).
//
// Driver around the reference's own v4 renderer.  oracle/build_ref.sh compiles this one translation
// unit with the reference's directory on the include path and REF_V4_BODY naming a temporary copy of
// demofox_path_tracing_optimization_v4.cpp lines 1-1556 (everything above the Win32 thread pool:
// RenderTile, OutputToScreen, mainImage, InitializeScene, InitializeCamera, Add*ToScene,
// UpdateTileInfo).  Being in the same translation unit, main() reaches the file's statics
// (iFrame, camera, scene, WorkData).  What one run does is what one process of the reference host
// does through DemofoxRenderOptV4 (:1696-1721) with its tiles taken in flat order by one thread:
//
//   InitializeCamera(); InitializeScene();                         (:1643-1653)
//   per frame: iFrame += 1.0f;                                      (:1703)
//              for each flat tile: RenderTile, then OutputToScreen  (:1557-1565)
//
// Usage: ref_v4 key=value ...
//   out=FILE            result file (layout below)                        required
//   w= h= tw= th=       image and tile size (w, tw multiples of 8; tw | w, th | h)
//   frames=N            calls (default 1)       frame0=F   iFrame before the first call (default 0)
//   env=FILE ew= eh=    env map, raw f32 RGB rows (six stacked faces for the cubemap build)
//   scene=FILE          replace InitializeScene's objects through Add*ToScene (layout below)
//   cam=px,py,pz,dist   camera.Position / camera.Distance
//   screen=1            also run OutputToScreen
//   dump=X,Y            print pixel (X, Y)'s accumulator after every frame (for locating a difference)
//
// Result file: i32 w, h, tw, th, has_screen; f32 iFrame; f32 acc[w*h*3] (the reference's tiled
// planar-8 layout, as RenderTile wrote it); u32 screen[w*h] if has_screen.
// Scene file: i32 nmat, nquads, nspheres; nmat x 17 f32 (SceneMaterial's member order);
// nquads x 12 f32 (V0 V1 V2 V3); nspheres x 4 f32 (centre, radius).
#include "ref_v4_shim.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include REF_V4_BODY
#include "texture.cpp"

static std::vector<float> read_f32(const char* path, size_t n)
{
    std::vector<float> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(float), n, f) != n) {
        fprintf(stderr, "ref_v4: cannot read %zu f32 from %s\n", n, path);
        exit(2);
    }
    fclose(f);
    return v;
}

static void load_scene(const char* path)
{
    FILE* f = fopen(path, "rb");
    int32_t n[3];
    if (!f || fread(n, sizeof(int32_t), 3, f) != 3 || n[0] < 0 || n[0] > MAX_MATERIALS || n[1] < 0 || n[2] < 0 ||
        n[1] > MAX_OBJECTS || n[2] > MAX_OBJECTS) {
        fprintf(stderr, "ref_v4: bad scene file %s\n", path);
        exit(2);
    }
    std::vector<float> d((size_t)n[0] * 17 + (size_t)n[1] * 12 + (size_t)n[2] * 4);
    if (fread(d.data(), sizeof(float), d.size(), f) != d.size()) {
        fprintf(stderr, "ref_v4: short scene file %s\n", path);
        exit(2);
    }
    fclose(f);
    // an empty scene: the counts back to zero and the material table cleared
    scene.NumQuadObjects = scene.NumSphereObjects = scene.NumMaterials = 0;
    memset(&scene.materials, 0, sizeof(scene.materials));
    const float* p = d.data();
    for (int i = 0; i < n[0]; ++i, p += 17) {
        SceneMaterial m;
        m.albedo = f32x3{p[0], p[1], p[2]};
        m.emissive = f32x3{p[3], p[4], p[5]};
        m.specularChance = p[6];
        m.specularRoughness = p[7];
        m.specularColor = f32x3{p[8], p[9], p[10]};
        m.IOR = p[11];
        m.refractionChance = p[12];
        m.refractionRoughness = p[13];
        m.refractionColor = f32x3{p[14], p[15], p[16]};
        AddMaterialToScene(scene, m);
    }
    for (int i = 0; i < n[1]; ++i, p += 12) {
        QuadSceneObject q{ 0 };   // as InitializeScene's own objects (:1415)
        q.V0 = set1x3_ps(p[0], p[1], p[2]);
        q.V1 = set1x3_ps(p[3], p[4], p[5]);
        q.V2 = set1x3_ps(p[6], p[7], p[8]);
        q.V3 = set1x3_ps(p[9], p[10], p[11]);
        AddQuadObjectToScene(scene, q);
    }
    for (int i = 0; i < n[2]; ++i, p += 4) {
        SphereSceneObject s;
        s.PositionAndRadius = set1x4_ps(p[0], p[1], p[2], p[3]);
        AddSphereObjectToScene(scene, s);
    }
}

int main(int argc, char** argv)
{
    std::string out, envf, scenef;
    int w = 0, h = 0, tw = 0, th = 0, frames = 1, ew = 0, eh = 0, screen = 0, dx = -1, dy = -1;
    float frame0 = 0.f, cam[4];
    bool have_cam = false;
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        const char* eq = strchr(a, '=');
        if (!eq) { fprintf(stderr, "ref_v4: bad argument %s\n", a); return 2; }
        const std::string k(a, eq - a), v(eq + 1);
        if (k == "out") out = v;
        else if (k == "env") envf = v;
        else if (k == "scene") scenef = v;
        else if (k == "w") w = atoi(v.c_str());
        else if (k == "h") h = atoi(v.c_str());
        else if (k == "tw") tw = atoi(v.c_str());
        else if (k == "th") th = atoi(v.c_str());
        else if (k == "ew") ew = atoi(v.c_str());
        else if (k == "eh") eh = atoi(v.c_str());
        else if (k == "frames") frames = atoi(v.c_str());
        else if (k == "frame0") frame0 = (float)atof(v.c_str());
        else if (k == "screen") screen = atoi(v.c_str());
        else if (k == "cam") have_cam = sscanf(v.c_str(), "%f,%f,%f,%f", &cam[0], &cam[1], &cam[2], &cam[3]) == 4;
        else if (k == "dump") sscanf(v.c_str(), "%d,%d", &dx, &dy);
        else { fprintf(stderr, "ref_v4: unknown key %s\n", k.c_str()); return 2; }
    }
    if (out.empty() || w <= 0 || h <= 0 || tw <= 0 || th <= 0 || w % 8 || tw % 8 || w % tw || h % th || frames < 0 ||
        (w / tw) * (h / th) > NumMaxThreads) {
        fprintf(stderr, "ref_v4: out= w= h= tw= th= are required (w, tw multiples of 8; tw | w; th | h)\n");
        return 2;
    }
    std::vector<float> env;
    texture tex;
    if (!envf.empty()) {
        if (ew <= 0 || eh <= 0) { fprintf(stderr, "ref_v4: env= needs ew= eh=\n"); return 2; }
        env = read_f32(envf.c_str(), (size_t)ew * eh * 3);
        tex.Data = env.data();
        tex.Width = ew;
        tex.Height = eh;
        tex.Components = 3;
    }

    InitializeCamera();
    InitializeScene();
    if (!scenef.empty()) load_scene(scenef.c_str());
    if (have_cam) {
        camera.Position = set1x3_ps(cam[0], cam[1], cam[2]);
        camera.Distance = set1_ps(cam[3]);
    }
    iFrame = frame0;

    const size_t npix = (size_t)w * h;
    float* acc = (float*)aligned_alloc(64, (npix * 3 * sizeof(float) + 63) / 64 * 64);
    uint32_t* pix = (uint32_t*)aligned_alloc(64, (npix * sizeof(uint32_t) + 63) / 64 * 64);
    memset(acc, 0, npix * 3 * sizeof(float));
    memset(pix, 0, npix * sizeof(uint32_t));

    const int ntx = w / tw, nty = h / th;
    UpdateTileInfo(acc, w, h, ntx, nty, tw, th, 3, tex, pix);
    for (int f = 0; f < frames; ++f) {
        iFrame += 1.0f;
        for (int t = 0; t < ntx * nty; ++t) {
            RenderTile(WorkData[t].BufferInfo, WorkData[t].TileInfo, WorkData[t].Texture);
            if (screen) OutputToScreen(WorkData[t].BufferInfo, WorkData[t].TileInfo, WorkData[t].ScreenBufferData);
        }
        if (dx >= 0 && dx < w && dy >= 0 && dy < h) {
            const size_t tile = (size_t)(dy / th) * th * w * 3 + (size_t)(dx / tw) * tw * th * 3;
            const size_t grp = tile + ((size_t)(dy % th) * (tw / 8) + (size_t)(dx % tw) / 8) * 24 + (size_t)dx % 8;
            printf("frame %.1f pixel (%d,%d): %.9g %.9g %.9g\n", iFrame, dx, dy, acc[grp], acc[grp + 8], acc[grp + 16]);
        }
    }

    FILE* fo = fopen(out.c_str(), "wb");
    if (!fo) { fprintf(stderr, "ref_v4: cannot write %s\n", out.c_str()); return 2; }
    const int32_t hdr[5] = {w, h, tw, th, screen ? 1 : 0};
    const float fr = iFrame;
    fwrite(hdr, sizeof(hdr), 1, fo);
    fwrite(&fr, sizeof(fr), 1, fo);
    fwrite(acc, sizeof(float), npix * 3, fo);
    if (screen) fwrite(pix, sizeof(uint32_t), npix, fo);
    fclose(fo);
    free(acc);
    free(pix);
    return 0;
}
