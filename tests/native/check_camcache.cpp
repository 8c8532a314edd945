// tests/native/check_camcache.cpp -- host check of the camera-hit cache's record format and size rule
// (csrc/pt_camcache.h, shared by the kernels and the host layer).
// usage: check_camcache     exit 0 iff every check holds
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pt_camcache.h"

static int fails = 0;
#define CHECK(c) \
    do { \
        if (!(c)) { \
            printf("FAILED line %d: %s\n", __LINE__, #c); \
            ++fails; \
        } \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

int main()
{
    // the round trip: every primitive and the miss, both flags, both fallback bits, distances
    // including c_superFar (10000), a denormal, -0 and a NaN pattern
    const float dist[] = {10000.0f, 0.0f, -0.0f, 1.0f, 17.25f, 1e-42f, 9999.999f};
    uint32_t db[8];
    for (int i = 0; i < 7; ++i) db[i] = bits(dist[i]);
    db[7] = 0x7fc12345u;
    for (uint32_t b : db)
        for (int id = -1; id <= 8; ++id)
            for (int flag = 0; flag <= 1; ++flag)
                for (int fb = 0; fb <= 1; ++fb) {
                    const unsigned long long r = pt_cam_pack(b, id, flag, fb);
                    CHECK(pt_cam_best_bits(r) == b);
                    CHECK(pt_cam_id(r) == id);
                    CHECK(pt_cam_flag(r) == flag);
                    CHECK(pt_cam_fb(r) == fb);
                }
    // records differ when any field differs (the counted launches' self-check compares whole records)
    CHECK(pt_cam_pack(db[3], 2, 0, 0) != pt_cam_pack(db[3], 3, 0, 0));
    CHECK(pt_cam_pack(db[3], 2, 0, 0) != pt_cam_pack(db[3], 2, 1, 0));
    CHECK(pt_cam_pack(db[3], 2, 0, 0) != pt_cam_pack(db[3], 2, 0, 1));
    CHECK(pt_cam_pack(db[3], 2, 0, 0) != pt_cam_pack(db[4], 2, 0, 0));
    // the buffer's initial state (memset 0xff) reads as a miss
    CHECK(pt_cam_id(~0ull) == -1);
    static_assert(sizeof(unsigned long long) == 8, "one 8-byte record per pixel");

    // the size rule: 8 bytes per pixel of whole 8x8 tiles, at most 128 MiB
    const auto tiles = [](uint32_t w, uint32_t h) { return ((w + 7) / 8) * ((h + 7) / 8); };
    CHECK(pt_cam_cache_bytes(tiles(1920, 1080)) == 16588800u);
    CHECK(pt_cam_cache_fits(tiles(1920, 1080)));
    CHECK(pt_cam_cache_bytes(tiles(3840, 2160)) == 66355200u);
    CHECK(pt_cam_cache_fits(tiles(3840, 2160)));
    CHECK(!pt_cam_cache_fits(tiles(7680, 4320)));
    CHECK(pt_cam_cache_fits(262144u) && !pt_cam_cache_fits(262145u));   // exactly 128 MiB / one tile more
    CHECK(pt_cam_cache_bytes(0x3fffffffu) == (size_t)0x3fffffffu * 512u);   // (no 32-bit overflow)

    // which geometries get one: the diffuse kernels' (kind 0) below the cap, while switched on
    CHECK(pt_cam_cache_wanted(true, 0, tiles(1920, 1080)));
    CHECK(!pt_cam_cache_wanted(false, 0, tiles(1920, 1080)));
    CHECK(!pt_cam_cache_wanted(true, 1, tiles(1920, 1080)) && !pt_cam_cache_wanted(true, 2, 600u));   // v4: jittered camera
    CHECK(!pt_cam_cache_wanted(true, 0, tiles(7680, 4320)));

    if (fails) return 1;
    printf("ok\n");
    return 0;
}
