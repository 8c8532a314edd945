// pt_v4_tile_pool.inc -- the body of the v4 per-tile pool kernels (pt_v4.hip includes it inside
// pt_v4_kernel, pt_v4_views_kernel, pt_v4_scenes_kernel, pt_v4_envs_kernel, pt_v4_batch_kernel and
// pt_v4_batch_stats_kernel, which declare ENV, LAYOUT, COUNT, DEF, FEXP, DFL, PRESENT, VIEWS, SCENES, ENVS, FRAMES,
// STATS, the kernel arguments job and sc, `cam`, the views arguments `va`, the scenes arguments `sa`, the view's
// scene `srec`, the envs arguments `ea`, the frame ranges `fa` and the statistics records `sta`).
    // SCENES: no block-wide material table (each wave follows its own view's scene: srec.mat / srec.mx).
    // SLDS (the A/B build PT_V4_SCENES_LDS=1): a table per wave in LDS, refilled when the wave takes a tile,
    // paid for by a shorter env miss queue, so that the block stays within 25 LDS granules.
    constexpr bool SLDS = SCENES && PT_V4_SCENES_LDS != 0;
    constexpr int kQ = SLDS ? 24 : kEnvQ;   // entries of the env miss queue
    constexpr int kMatRows = SCENES ? (SLDS ? kWaves * PT_V4_MAX_OBJECTS : 1) : PT_V4_MAX_OBJECTS;
    __shared__ float s_col[kWaves][kChunk * 64 * 3];
    __shared__ PtV4Mat s_mat[kMatRows];
    __shared__ float4 s_sc[DEF ? pt_v4_default::kSpheres : 1];   // default scene: sphere centre, radius
    __shared__ MatX s_mx[kMatRows];                                 // per-material constants (mat_consts)
    constexpr bool DEFER = ENV != PT_V4_ENV_NONE_;
    __shared__ float4 s_qd[DEFER ? kWaves : 1][DEFER ? kQ : 1];   // env dir, rng
    __shared__ float4 s_qt[DEFER ? kWaves : 1][DEFER ? kQ : 1];   // throughput, colour slot
    if constexpr (!SCENES) {
    for (int t = threadIdx.x; t < PT_V4_MAX_OBJECTS * 17; t += 64 * kWaves)
        reinterpret_cast<float*>(s_mat)[t] = reinterpret_cast<const float*>(sc.mat)[t];
    __syncthreads();
    if (threadIdx.x < PT_V4_MAX_OBJECTS) s_mx[threadIdx.x] = mat_consts(s_mat[threadIdx.x]);
    }
    if (DEF && threadIdx.x < pt_v4_default::kSpheres) {
        const float* c = pt_v4_default::kSphere[threadIdx.x];
        s_sc[threadIdx.x] = make_float4(c[0], c[1], c[2], c[3]);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    pt_queue_zero_next(job.queue_next);   // (pt_tile_queue.h)
    const int tiles_x = (job.ncols + 7) >> 3;
    const int ntiles = tiles_x * ((job.nrows + 7) >> 3);
    float* const col = s_col[wv];
    const size_t cs = (LAYOUT == PT_LAYOUT_INTERLEAVED) ? 1u : 8u;
    Tex tex{job.env, job.env_w, job.env_h};   // (ENVS: the tile's view's texture, taken below; the job's is null)
    const bool random = DFL || job.random_jitter != 0, rejection = DFL || job.rejection != 0;
    const int B = job.num_bounces;
    const float W = (float)job.width, H = (float)job.height;
    const float rW = rcp(W), rH = rcp(H);
    unsigned long long n_seg = 0, n_esc = 0, n_slots = 0, n_fb = 0, n_sky = 0;

    // persistent waves: 8x8 tiles from the launch's queue (pt_tile_queue.h), longest first when the
    // geometry has a schedule
    constexpr uint32_t kNone = PtTileQueue<kWaves>::kNone;
    // (VIEWS: every view's tiles, in view order; the host keeps ntiles x nviews within PT_TILE_MASK)
    PtTileQueue<kWaves> tq(job.queue, job.order, job.units, job.nunits,
                           VIEWS ? (uint32_t)ntiles * (uint32_t)va.nviews : (uint32_t)ntiles, wv);
    uint32_t tile = kNone, next_tile = kNone;
    tile = tq.first(job.err);   // (the whole wave: uniform, scalar registers)
    tile = __builtin_amdgcn_readfirstlane(tile);
    while (tile != kNone) {
    // (this kernel's schedules hold whole tiles: pt_capi.cpp v4_launch)
    int vtile = (int)pt_entry_tile(tile);   // the tile inside its image
    uint32_t view = 0;                      // VIEWS: the entry's view (its slices start at view * nrows * width pixels)
    if constexpr (VIEWS) {
        // the entry is (view, tile): the wave may have come from another view's tile, so the camera
        // is taken anew here -- origin, distance, has_sky() and the rectangles all follow `cam`
        view = (uint32_t)vtile / (uint32_t)ntiles;
        vtile -= (int)(view * (uint32_t)ntiles);
        if (!PT_GUARD(job.err, view < (uint32_t)va.nviews, PT_G_VIEW, view)) view = 0;   // (checked build: reported)
        cam.take(va.table, view);
        if (!PT_GUARD(job.err, cam.nrects <= PT_V4_SKYWIN_MAX, PT_G_VIEW, 0x80000000u | view)) cam.nrects = -1;
    }
    if constexpr (SCENES) {
        // and so is the scene: the record pointer, both object counts and the material pointers are
        // replaced (a scene with fewer objects, or none, after one with more; equal geometry with other
        // materials).  The index comes from the view's entry of the mapping, a scalar load like the record's.
        uint32_t scene = (uint32_t)((const __attribute__((address_space(4))) int32_t*)sa.scene_of_view)[view];
        if (!PT_GUARD(job.err, scene < (uint32_t)sa.nscenes, PT_G_SCENE, scene)) scene = 0;   // (checked build: reported)
        srec.take(sa.table, scene);
        if (!PT_GUARD(job.err, srec.nquads >= 0 && srec.nspheres >= 0 && srec.nquads + srec.nspheres <= PT_V4_MAX_OBJECTS,
                      PT_G_SCENE, 0x80000000u | scene))
            srec.nquads = srec.nspheres = 0;
        if constexpr (SLDS) {
            // this wave's rows only, written and read by this wave alone: its reads of the previous tile's
            // rows are done (program order), the refill is fenced like s_col's
            float* const wm = reinterpret_cast<float*>(s_mat + wv * PT_V4_MAX_OBJECTS);
            float* const wx = reinterpret_cast<float*>(s_mx + wv * PT_V4_MAX_OBJECTS);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int t = lane; t < PT_V4_MAX_OBJECTS * 17; t += 64) wm[t] = reinterpret_cast<const float*>(srec.mat)[t];
            if (lane < PT_V4_MAX_OBJECTS * PT_V4_MATX_FLOATS) wx[lane] = reinterpret_cast<const float*>(srec.mx)[lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            srec.mat = s_mat + wv * PT_V4_MAX_OBJECTS;
            srec.mx = s_mx + wv * PT_V4_MAX_OBJECTS;
        }
    }
    if constexpr (ENVS) {
        // and so is the texture: pointer, width and height are replaced together, from one record read
        // through the constant address space at a wave-uniform address (scalar loads, scalar registers;
        // texel_at / texel_rn clamp with w * h, so dimensions of another texture would index past this one).
        // Invariant: no deferred miss survives a tile.  The entries of s_qd / s_qt carry a direction, an rng
        // and a slot but no texture; `resolve` reads this wave's current `tex`.  That is right only because
        // every chunk ends with drain(qn), before the wave leaves the tile and comes back here.
        uint32_t env = (uint32_t)((const __attribute__((address_space(4))) int32_t*)ea.env_of_view)[view];
        if (!PT_GUARD(job.err, env < (uint32_t)ea.nenvs, PT_G_ENV, env)) env = 0;   // (checked build: reported)
        const __attribute__((address_space(4))) PtV4EnvRec* const er = (const __attribute__((address_space(4))) PtV4EnvRec*)(ea.table + env);
        tex = Tex{er->data, er->w, er->h};
        if (!PT_GUARD(job.err, tex.w > 0 && tex.h > 0, PT_G_ENV, 0x80000000u | env)) tex.w = tex.h = 1;
    }
    // The tile's frame range: everything below that depends on the first frame or the frame count -- the
    // chunk loop and nf, the seed, the blend factor and BOTH tq.next conditions -- reads these two and
    // nothing else, so loop and queue cannot disagree about the count (exactly one tq.next per tile: in
    // the chunk with c0 < t_nframes <= c0 + kChunk, or after the loop when t_nframes <= 0).
    // (Without FRAMES they are the job's members, named where they are read -- `FRAMES ? view's : job's`
    // with a constant condition is the job's member itself -- so the other kernels keep their instructions.)
    uint32_t t_first = 0;
    int t_nframes = 0;
    if constexpr (FRAMES) {
        // the view's own range (a wave goes from a view of 9 frames to one of 1, of 0, of 17): ONE 8-byte
        // read through the constant address space at a wave-uniform address, so first frame and count are
        // of the same record (a stale first frame with a fresh count would render the right number of
        // frames from the wrong seeds) and both sit in scalar registers.  Nothing of it is block-shared.
        const uint64_t fr = *(const __attribute__((address_space(4))) uint64_t*)(fa.range_of_view + view);
        t_first = (uint32_t)fr;
        t_nframes = (int)(uint32_t)(fr >> 32);
        // (checked build: a bad record is reported and the view treated as one of 0 frames)
        if (!PT_GUARD(job.err, t_nframes >= 0 && t_first >= 1u && (uint64_t)t_first + (uint64_t)(uint32_t)t_nframes <= (1ull << 24),
                      PT_G_FRAMES, view))
            t_nframes = 0;
    }
    const int tcol = (vtile % tiles_x) * 8, trow = (vtile / tiles_x) * 8;
    uint32_t tile_work = 1;   // pool iterations of this tile (the schedule's cost)

    // this lane's pixel (phase C) and its accumulator
    const int px = job.col0 + tcol + (lane & 7), pr = trow + (lane >> 3);
    const bool pvalid = (tcol + (lane & 7)) < job.ncols && pr < job.nrows;
    float* acc_p = nullptr;
    V3 acc = v3(0.0f, 0.0f, 0.0f);
    if (pvalid) {
        // compact layouts index the buffer row; the tiled layout indexes the full image (global row)
        const int orow = LAYOUT == PT_LAYOUT_TILED_PLANAR8 ? job.row_start + pr * job.row_stride : pr;
        size_t pi = out_index<LAYOUT>(job, px, orow);
        if constexpr (VIEWS)   // (checked build: an element outside the view's slice is reported, element 0 used)
            if (!PT_GUARD(job.err, pi + 2 * cs < pixel_extent<LAYOUT>(job), PT_G_PIXEL, pi)) pi = 0;
        if constexpr (VIEWS) pi += (size_t)view * (size_t)job.nrows * (size_t)job.width * 3u;
        acc_p = job.buf + pi;
        // (a view of 0 frames: its accumulator is read, to pack its pixel, and never written)
        if (job.accumulate || (FRAMES && t_nframes <= 0)) acc = v3(acc_p[0], acc_p[cs], acc_p[2 * cs]);   // (:1233: only to blend; 0 frames: to pack)
    }

    for (int c0 = 0; c0 < (FRAMES ? t_nframes : job.nframes); c0 += kChunk) {
        const int nf = std::min(kChunk, (FRAMES ? t_nframes : job.nframes) - c0);
        const int total = 64 * nf;
        int next = 0;      // wave-uniform
        int item = -1;     // this lane's (pixel, frame) sample, -1 = none
        V3 pos, dir, T, ret;
        uint32_t rng = 0;
        int bounce = 0;
        int qn = 0;   // queued misses (DEFER), wave-uniform
        // a deferred miss: env(d) with the rng state r, fma'd with throughput t into colour slot k
        auto resolve = [&](V3 d, uint32_t r, V3 t, int k) {
            V3 amb = v3(0.0f, 0.0f, 0.0f);
            if (ENV == PT_V4_ENV_EQUIRECT_) amb = equirect(tex, d, random, r);
            if (ENV == PT_V4_ENV_CUBEMAP_) amb = cubemap(tex, d, random, r);
            float* o = col + k;
            const V3 rt = v3(fma_(amb.x, t.x, o[0]), fma_(amb.y, t.y, o[1]), fma_(amb.z, t.z, o[2]));   // :787
            o[0] = fma_(rt.x, 1.0f, 0.0f);   // :1127
            o[1] = fma_(rt.y, 1.0f, 0.0f);
            o[2] = fma_(rt.z, 1.0f, 0.0f);
        };
        // evaluate the queued misses [0, m), one per lane
        auto drain = [&](int m) {
            if (lane < m) {
                const float4 a = s_qd[DEFER ? wv : 0][lane], b = s_qt[DEFER ? wv : 0][lane];
                resolve(v3(a.x, a.y, a.z), __builtin_bit_cast(uint32_t, a.w), v3(b.x, b.y, b.z),
                        __builtin_bit_cast(int, b.w));
            }
        };
        for (;;) {
            // hand out items to idle lanes, in lane order
            const bool need = item < 0;
            const unsigned long long m = pt_ballot(need);
            if (need) {
                const int it = next + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (it < total) {
                    // frame-major (pixel-major, a pixel's frames on neighbouring lanes, measured
                    // 1-2.5 % slower here: the jittered camera rays share no bounce-0 origin)
                    const int p = it & 63, f = it >> 6;
                    const int X = job.col0 + tcol + (p & 7), rb = trow + (p >> 3);
                    if ((tcol + (p & 7)) < job.ncols && rb < job.nrows) {
                        item = f * 64 + p;   // colour slot order (phase C)
                        // mainImage :1092-1130
                        const int Y = job.row_start + rb * job.row_stride;
                        const uint32_t frame = (FRAMES ? t_first : job.frame_first) + (uint32_t)(c0 + f);
                        const int fyi = job.height - 1 - Y;
                        // 24 x 24-bit products: X, fyi, frame < 2^24 (C ABI), low words = the u32 products
                        rng = 1u | (__umul24((uint32_t)X, 1973u) + __umul24((uint32_t)fyi, 9277u) + __umul24(frame, 26699u));
                        const float jx = randf(rng) - 0.5f;
                        const float jy = randf(rng) - 0.5f;
                        const float tx = fma_(((float)X + jx) * rW, 2.0f, -1.0f);
                        float ty = fma_(((float)fyi + jy) * rH, 2.0f, -1.0f);
                        ty = ty * (rW * H);
                        dir = cam.ray(tx, ty);
                        pos = cam.position();
                        T = v3(1.0f, 1.0f, 1.0f);
                        ret = v3(0.0f, 0.0f, 0.0f);
                        bounce = 0;
                    }
                }
            }
            next += __builtin_popcountll(m);
            if (pt_ballot(item >= 0) == 0ull) break;
            ++tile_work;
            if (COUNT) n_slots += 64;
            bool queued = false;   // DEFER: this lane's item missed and goes to the queue
            int qslot = 0;
            // default scene: when every busy lane traces a camera ray that leaves the scene's
            // silhouette (sky_ray_v4), the wave skips TestSceneTrace -- the reference's miss
            // (the slope test runs only in iterations where every busy lane is at bounce 0: a wave-
            // uniform branch, instead of the test on every lane in every iteration)
            // any other (scene, camera): the same with its sky window (pt_v4_skywin.h), when it has one
            bool all_sky = false;
            if (cam.has_sky() && pt_ballot(item >= 0 && bounce != 0) == 0)
                all_sky = pt_ballot(item >= 0 && !cam.sky(dir)) == 0;
            if (item >= 0) {
                bool done = false;
                if constexpr (SCENES)   // the view's scene record and its material rows
                    v4_segment<ENV, COUNT, DEF, FEXP, DFL>(job, srec, srec.mat, srec.mx, s_sc, tex, random, rejection, B, all_sky,
                                                           pos, dir, T, ret, rng, bounce, done, queued, n_seg, n_esc, n_fb, n_sky);
                else
                v4_segment<ENV, COUNT, DEF, FEXP, DFL>(job, sc, s_mat, s_mx, s_sc, tex, random, rejection, B, all_sky, pos,
                                                       dir, T, ret, rng, bounce, done, queued, n_seg, n_esc, n_fb, n_sky);
                if (done) {
                    const int p = item & 63, f = item >> 6;
                    qslot = (f * 64 + p) * 3;
                    float* o = col + qslot;
                    if (DEFER && queued) {   // ret so far; the drain adds the env term
                        o[0] = ret.x;
                        o[1] = ret.y;
                        o[2] = ret.z;
                    } else {
                        // mainImage :1127: fmadd(color, 1/c_numRendersPerFrame, 0)
                        o[0] = fma_(ret.x, 1.0f, 0.0f);
                        o[1] = fma_(ret.y, 1.0f, 0.0f);
                        o[2] = fma_(ret.z, 1.0f, 0.0f);
                    }
                    item = -1;
                }
            }
            if (DEFER) {
                const unsigned long long qm = pt_ballot(queued);
                const int nq = __builtin_popcountll(qm);
                const V3 ed = ENV == PT_V4_ENV_EQUIRECT_ ? v3(-dir.x, dir.y, -dir.z) : dir;
                if (qn + nq > kQ) {
                    // overflow: one env pass over the whole wave -- the new misses in their own lanes,
                    // the other lanes each take one queued miss (the top `take` entries, so the rest
                    // stay in place).  At least kEnvQ + 1 lanes busy (min(qn + nq, 64)); the drain-or-
                    // new-batch choice this replaces ran 24-48 of the 64.
                    const int take = std::min(qn, 64 - nq);
                    const int r = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(~qm >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)~qm, 0u));
                    V3 d = ed, t = T;
                    uint32_t rr = rng;
                    int k = qslot;
                    bool act = queued;
                    if (!queued && r < take) {
                        const int e = qn - take + r;
                        const float4 a = s_qd[DEFER ? wv : 0][DEFER ? e : 0], b = s_qt[DEFER ? wv : 0][DEFER ? e : 0];
                        d = v3(a.x, a.y, a.z);
                        rr = __builtin_bit_cast(uint32_t, a.w);
                        t = v3(b.x, b.y, b.z);
                        k = __builtin_bit_cast(int, b.w);
                        act = true;
                    }
                    if (act) resolve(d, rr, t, k);
                    qn -= take;
                } else {
                    if (queued) {
                    const int k = qn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(qm >> 32),
                                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)qm, 0u));
                        s_qd[DEFER ? wv : 0][k] = make_float4(ed.x, ed.y, ed.z, __builtin_bit_cast(float, rng));
                        s_qt[DEFER ? wv : 0][k] = make_float4(T.x, T.y, T.z, __builtin_bit_cast(float, qslot));
                    }
                    qn += nq;
                }
            }
        }
        if (DEFER && qn > 0) drain(qn);
        if (c0 + kChunk >= (FRAMES ? t_nframes : job.nframes)) next_tile = tq.next(job.err);   // the last pool is done
        // all radiance of this chunk is in LDS (written by lanes of this wave)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (pvalid) {
            for (int f = 0; f < nf; ++f) {
                const float* c = col + (f * 64 + lane) * 3;
                if (job.accumulate) {   // ACCUMULATE_FRAMES 1: fmadd(blend_factor, color - last, last) :1233-1241
                    const float bf = rcp((float)((FRAMES ? t_first : job.frame_first) + (uint32_t)(c0 + f)) + 1.0f);   // :1200
                    acc = v3(fma_(bf, c[0] - acc.x, acc.x), fma_(bf, c[1] - acc.y, acc.y), fma_(bf, c[2] - acc.z, acc.z));
                } else {                // ACCUMULATE_FRAMES 0: the frame's colour is stored (:1245-1250)
                    acc = v3(c[0], c[1], c[2]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if ((FRAMES ? t_nframes : job.nframes) <= 0) next_tile = tq.next(job.err);   // no chunk ran
    if constexpr (STATS) {
        // How much the tile's displayed pixels moved (pt_v4.h PtV4Stats): each lane with a pixel packs the value
        // the launch found -- re-read here, the slice is untouched until the store below, so no old value lives
        // through the pool loop (and accumulate 0, which never loaded it, needs no other path) -- and the value it
        // is about to store; the wave reduces one register (pt_v4_stats.h) and one lane adds the tile's sums to
        // its view's record.  A lane without a pixel contributes 0.  The branch is wave-uniform (t_nframes is the
        // view's, in a scalar register): a view of 0 frames issues nothing and its record stays as the host
        // cleared it.
        if (t_nframes > 0) {
            uint32_t d = 0;
            if (pvalid)
                d = v4_stats_delta(pt_tone::pack<true, true>(acc_p[0], acc_p[cs], acc_p[2 * cs], true),
                                   pt_tone::pack<true, true>(acc.x, acc.y, acc.z, true));
            const uint32_t n_changed = (uint32_t)__builtin_popcountll(pt_ballot(d != 0u));
            d = v4_stats_wave(d);
            // (checked build: a record beyond the nviews records is reported and nothing added)
            if (lane == 0 && PT_GUARD(job.err, view < (uint32_t)va.nviews, PT_G_STATS, view))
                v4_stats_commit(sta.of_view + view, d & 0xffffu, n_changed, d >> 16);
        }
    }
    if (pvalid) {
        if (!FRAMES || t_nframes > 0) {
            acc_p[0] = acc.x;
            acc_p[cs] = acc.y;
            acc_p[2 * cs] = acc.z;
        }
        v4_present<PRESENT>(job, px, job.row_start + pr * job.row_stride, acc);
        if constexpr (VIEWS) {
            // the view's packed pixels, job rows (a device job: col0 0, ncols == width), when asked for
            const size_t po = (size_t)(uint32_t)pr * (uint32_t)job.width + (uint32_t)px;
            if (va.pix && PT_GUARD(job.err, po < (size_t)job.nrows * (size_t)job.width, PT_G_PIXOUT, po))
                va.pix[(size_t)view * (size_t)job.nrows * (size_t)job.width + po] = pt_tone::pack<true, true>(acc.x, acc.y, acc.z, job.pix_xrgb != 0);
        }
    }
    if constexpr (VIEWS) (void)tile_work;   // (views launches are unscheduled: no cost record, pt_launch_v4_batched)
    else if (job.cost && lane == 0) pt_record_cost(job.cost, tile, (uint32_t)ntiles, tile_work);
    tile = __builtin_amdgcn_readfirstlane(next_tile);
    }
    tq.report(job.err);   // (a schedule entry outside the launch, pt_tile_queue.h)
    if (COUNT) {
        // per-lane counts summed over the wave by lane 0's atomics
        for (int off = 32; off > 0; off >>= 1) {
            n_seg += __shfl_down(n_seg, off);
            n_esc += __shfl_down(n_esc, off);
            n_fb += __shfl_down(n_fb, off);
            n_sky += __shfl_down(n_sky, off);
        }
        if (lane == 0) {
            atomicAdd(&job.counters[0], n_seg);
            atomicAdd(&job.counters[2], n_esc);
            atomicAdd(&job.counters[3], n_slots);
            atomicAdd(&job.counters[4], n_fb);
            atomicAdd(&job.counters[5], n_sky);
        }
    }
