// hrn_ctx, part 5: what a call keeps on the handle outside the planned workspace -- the guard that serialises calls on different
// streams (CallGuard, CallScope), the device arrays a call rewrites (CallScratch), the pinned staging ring their uploads go through
// (PinnedImage) and the one frame every entry that keeps such an array runs in (CallFrame: reserve, enter, upload, leave, in that
// order); then the Gaussian tables of the scoring.  Outside this file an entry meets a CallScratch only through a CallFrame, and a
// CallScope only on `pass`.  Included inside struct hrn_ctx (hrnet_mi355.cpp).

    // One handle, one copy of everything a call writes: calls on DIFFERENT streams must not overlap on it.  Whoever uses the guarded
    // thing records `done` behind its last kernel (leave); a call on another stream than the previous one waits for that event first
    // (enter).  Same stream: ordered anyway, nothing is waited for.
    struct CallGuard {
        hipEvent_t done = nullptr;
        hipStream_t stream = nullptr;   // of the last user
        bool enter(hrn_ctx *h, hipStream_t s) {
            if (!done) return h->hip_ok(hipEventCreateWithFlags(&done, hipEventDisableTiming), "hipEventCreate");
            return stream == s || h->hip_ok(hipStreamWaitEvent(s, done, 0), "hipStreamWaitEvent");
        }
        bool leave(hrn_ctx *h, hipStream_t s) {
            stream = s;
            return h->hip_ok(hipEventRecord(done, s), "hipEventRecord");
        }
        void release() {
            if (done) (void)hipEventDestroy(done);
            done = nullptr, stream = nullptr;
        }
    };

    // A device array of the handle that each call rewrites, with its guard.  reserve() before enter(): growing waits on the host
    // until the last user's kernels have read the old array.  A family with several arrays enters the guard of its first one and
    // names it as `readers` when it reserves the others (CallFrame, below, does both).
    struct CallScratch : CallGuard {
        char *ptr = nullptr;
        size_t bytes = 0;
        template <class T>
        T *as() const { return (T *)ptr; }
        // at least `need` bytes; a grow allocates `cap` (>= need: the caller's growth rule)
        bool reserve(hrn_ctx *h, size_t need, size_t cap, const char *what, CallGuard *readers = nullptr) {
            if (need <= bytes) return true;
            if (!readers) readers = this;
            if (readers->done && !h->hip_ok(hipEventSynchronize(readers->done), "hipEventSynchronize")) return false;
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr, bytes = 0;
            if (!h->hip_ok(hipMalloc((void **)&ptr, cap), what)) return false;
            bytes = cap;
            return true;
        }
        void release() {
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr, bytes = 0;
            CallGuard::release();
        }
    };

    // enter() .. leave() on EVERY exit (ADVICE r3): kernels and copies already queued by a call that failed half-way must be covered
    // by `done` too, or the next call on another stream could rewrite what they still read.  A null guard guards nothing.
    struct CallScope {
        hrn_ctx *h;
        CallGuard *g;
        hipStream_t s;
        bool entered, left = false;
        CallScope(hrn_ctx *h_, CallGuard *g_, hipStream_t s_) : h(h_), g(g_), s(s_), entered(!g_ || g_->enter(h_, s_)) {}
        CallScope(const CallScope &) = delete;
        bool leave() {
            left = true;
            return entered && (!g || g->leave(h, s));
        }
        ~CallScope() {   // a failure exit: the call's own error text stays
            if (g && entered && !left) g->stream = s, (void)hipEventRecord(g->done, s);
        }
    };

    CallGuard pass;            // the workspace: every entry point that runs a pass
    CallScratch rs_taps;       // hrn_resize_frames: tap tables of the last (frame size, interpolation)
    CallScratch pre_tmp, pre_params, pre_yuv;   // crop pre-path: intermediates, CropParams and (YUV frames) a YuvSource per person; pre_tmp's guard
    CallScratch warp_params;   // hrn_warp_crops: the inverse matrices
    CallScratch score_joints;  // hrn_score_heatmaps, hrn_generate_targets: the per-(crop, joint) records
    CallScratch draw_table, draw_records;   // hrn_draw_poses: the call's table (canvases, people by canvas, colours, skeleton) and the
                                            // per-person records the build launch writes; draw_table's guard
    CallScratch assoc_buf;     // hrn_associate_people_dev: the problem table of a call with several problems, then the costs and
                               // similarities the kernel keeps between its phases
    CallScratch tracks_buf;    // hrn_track_people_dev: the stream table of a call with several streams, then per stream the costs,
                               // the similarities and (coast) the compared state the kernel keeps between its phases
    CallScratch nms_table;     // hrn_pose_nms_dev: the problem table of a call with several problems
    CallScratch eval_buf;      // hrn_keypoint_eval_dev: the image table, then the set-wide order of the slots
    CallScratch trk_table;     // the tracking link: the call's host table (frame sizes per person; frame table and frame index)
    CallScratch lb_table;      // hrn_letterbox_frames(_yuv): the frame records of a call with several frames
    CallScratch det_table;     // hrn_detections_to_frame_dev: the frame records of a call with several frames
    CallScratch rot_table;     // hrn_rotate_frames: the plane records of a call with several frames
    CallScratch rot_people;    // hrn_rotate_people_dev: the frame sizes / codes of a call that has them per person
    CallScratch yuvout_table;  // hrn_bgr_to_yuv_frames: the frame records of a call with several frames
    CallScratch dnms_buf;      // hrn_detector_nms_dev: the candidates of the scoring launch, then the chunk counts and their scan
    CallScratch tmp_table;     // hrn_filter_poses_dev: every person's segment of the previous people, of a call with several problems

    // pinned host image of one call's tables (the async uploads read it after the call returned); kPreRing images in rotation,
    // each rewritten only after the upload that last read it has completed
    static constexpr int kPreRing = 4;
    char *pre_pin[kPreRing] = {nullptr, nullptr, nullptr, nullptr};
    size_t pre_pin_bytes[kPreRing] = {0, 0, 0, 0};
    hipEvent_t pre_landed[kPreRing] = {nullptr, nullptr, nullptr, nullptr};
    unsigned pre_ring_next = 0;
    struct PinnedImage {
        char *ptr = nullptr;
        unsigned slot = 0;   // of the ring
        size_t bytes = 0;
        explicit operator bool() const { return ptr != nullptr; }
        template <class T>
        T *as(size_t at = 0) const { return (T *)(ptr + at); }
    };
    // the next image of the ring, `need` bytes, free to be rewritten (empty + err on failure).  It needs no guard: an entry that
    // validates while it fills takes it first and may still refuse; CallFrame::upload sends it
    PinnedImage image(size_t need) {
        const unsigned ring = pre_ring_next++ % kPreRing;
        if (pre_landed[ring]) {
            if (!hip_ok(hipEventSynchronize(pre_landed[ring]), "hipEventSynchronize")) return {};
        } else if (!hip_ok(hipEventCreateWithFlags(&pre_landed[ring], hipEventDisableTiming), "hipEventCreate")) {
            return {};
        }
        if (need > pre_pin_bytes[ring]) {
            if (pre_pin[ring]) (void)hipHostFree(pre_pin[ring]);
            pre_pin[ring] = nullptr, pre_pin_bytes[ring] = 0;
            const size_t cap = std::max<size_t>(need * 2, 4096);
            if (!hip_ok(hipHostMalloc((void **)&pre_pin[ring], cap, hipHostMallocDefault), "hipHostMalloc(crop params)")) return {};
            pre_pin_bytes[ring] = cap;
        }
        return {pre_pin[ring], ring, need};
    }

    // One call on the arrays of one family.  The constructor reserves every array (a grow waits on the host for the last reader,
    // so it comes first), then enters the guard of the first one on s; the others are reserved against that guard.  Only an entered
    // frame hands out device pointers or queues uploads, and it leaves as CallScope does: leave() on success, the destructor on
    // every other exit.  A first need of 0 bytes -- the one problem that travels in the kernel arguments -- reserves, guards and
    // uploads nothing and costs no HIP call.
    struct Want {
        CallScratch *array;
        size_t need, cap;   // cap: what a grow allocates -- `need` (exact), twice(need, floor), or a rule of the entry's own
        const char *what;
    };
    static size_t twice(size_t need, size_t floor) { return std::max(need * 2, floor); }
    struct CallFrame {
        hrn_ctx *h;
        hipStream_t s;
        CallScratch *first;
        bool reserved;
        CallScope scope;
        bool failed = false;   // an upload
        CallFrame(hrn_ctx *h_, hipStream_t s_, std::initializer_list<Want> wants)
            : h(h_), s(s_), first(wants.begin()->array), reserved(reserve(h_, wants)),
              scope(h_, reserved && wants.begin()->need ? first : nullptr, s_) {}
        static bool reserve(hrn_ctx *h, std::initializer_list<Want> wants) {
            if (!wants.begin()->need) return true;
            for (const Want &w : wants)
                if (!w.array->reserve(h, w.need, w.cap, w.what, wants.begin()->array)) return false;
            return true;
        }
        bool guarded() const { return scope.g != nullptr; }
        bool ok() const { return reserved && scope.entered && !failed; }   // false: the entry returns 6
        bool leave() { return ok() && scope.leave(); }
        template <class T = char>
        T *dev(const CallScratch &a, size_t at = 0) const { return ok() ? (T *)(a.ptr + at) : nullptr; }
        template <class T = char>
        T *dev(size_t at = 0) const { return dev<T>(*first, at); }
        // pieces of `img` to the device on s, then the event that lets the image be rewritten (a null destination: skipped; a
        // destination may be the caller's own)
        struct Piece {
            void *dst;
            const void *src;
            size_t bytes;
            const char *what;
        };
        bool upload(const PinnedImage &img, std::initializer_list<Piece> pieces) {
            if (!ok()) return false;
            for (const Piece &p : pieces)
                if (p.dst && !h->hip_ok(hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyHostToDevice, s), p.what)) return !(failed = true);
            return !(failed = !h->hip_ok(hipEventRecord(h->pre_landed[img.slot], s), "hipEventRecord"));
        }
        // the first `bytes` of `img` into the first array at `at`; where they lie, or nullptr (not guarded, or failed: ok())
        template <class T = char>
        T *upload(const PinnedImage &img, size_t bytes, const char *what, size_t at = 0) {
            return guarded() && upload(img, {{first->ptr + at, img.ptr, bytes, what}}) ? (T *)(first->ptr + at) : nullptr;
        }
        // `count` records through an image that fill(T *) writes: the table on the device, or nullptr -- not guarded (the one
        // record goes into the kernel arguments), or failed (ok())
        template <class T, class Fill>
        const T *table(size_t count, const char *what, const Fill &fill) {
            if (!guarded() || !ok()) return nullptr;
            const PinnedImage img = h->image(count * sizeof(T));
            if (!img) return failed = true, nullptr;
            fill(img.as<T>());
            return upload<T>(img, count * sizeof(T), what);
        }
        template <class T>
        const T *table(const T *records, size_t count, const char *what) {
            return table<T>(count, what, [&](T *out) { memcpy(out, records, count * sizeof(T)); });
        }
    };
    // the pre-path's frame for n people: `tmp_bytes` of intermediates (exact: they can be large), n records (and n YUV sources)
    struct PreFrame : CallFrame {
        PreFrame(hrn_ctx *h, size_t tmp_bytes, size_t n, bool yuv, hipStream_t s)
            : CallFrame(h, s, {{&h->pre_tmp, tmp_bytes, tmp_bytes, "hipMalloc(pre-path scratch)"},
                               {&h->pre_params, n * sizeof(CropParams), n * sizeof(CropParams), "hipMalloc(crop params)"},
                               {&h->pre_yuv, yuv ? n * sizeof(YuvSource) : 0, n * sizeof(YuvSource), "hipMalloc(YUV sources)"}}) {}
    };

    // scoring: the Gaussian tables g[d2] = float32(exp(-d2 / (2 sigma^2))), d2 = 0 .. 2 t^2, by t = 3 sigma
    std::map<int, float *> score_tables;
    const float *score_table(int t, double sigma) {   // built in fp64 and rounded once, on the first call with this sigma
        auto it = score_tables.find(t);
        if (it != score_tables.end()) return it->second;
        std::vector<float> g((size_t)2 * t * t + 1);
        for (size_t d2 = 0; d2 < g.size(); ++d2) g[d2] = (float)std::exp(-(double)d2 / (2.0 * sigma * sigma));
        float *dev = nullptr;
        if (!hip_ok(hipMalloc((void **)&dev, g.size() * sizeof(float)), "hipMalloc(Gaussian table)")) return nullptr;
        if (!hip_ok(hipMemcpy(dev, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(Gaussian table)")) {
            (void)hipFree(dev);
            return nullptr;
        }
        return score_tables[t] = dev;
    }

    void free_scratch() {
        for (CallScratch *c : {&rs_taps, &pre_tmp, &pre_params, &pre_yuv, &warp_params, &score_joints, &draw_table, &draw_records, &assoc_buf, &tracks_buf,
                               &nms_table, &eval_buf, &trk_table, &lb_table, &det_table, &rot_table, &rot_people, &yuvout_table, &dnms_buf, &tmp_table})
            c->release();
        pass.release();
        for (auto &kv : score_tables) (void)hipFree(kv.second);
        score_tables.clear();
        for (int k = 0; k < kPreRing; ++k) {
            if (pre_pin[k]) (void)hipHostFree(pre_pin[k]);
            if (pre_landed[k]) (void)hipEventDestroy(pre_landed[k]);
            pre_pin[k] = nullptr, pre_landed[k] = nullptr, pre_pin_bytes[k] = 0;
        }
    }
