// struct hrn_ctx, part: device memory; block maps / unit lists of the grouped launches per micro-batch size; descriptors.
// Included INSIDE the struct body by hrnet_mi355.cpp (member functions defined in place; one type, split by concern:
// ctx_plan / ctx_memory / ctx_weights / ctx_run).
    // ---------------------------------------------------------------- device memory
    bool hip_ok(hipError_t e, const char *what) {
        if (e == hipSuccess) return true;
        err = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    }
    // true (and the text) on a handle made with device_id < 0: the entries that would touch the device refuse it
    bool refuse_plan_only() {
        if (plan_only) err = "plan-only handle (device_id < 0): there is no CPU compute path";
        return plan_only;
    }

    bool allocate() {
        workspace_bytes = 0;
        for (auto &b : buffers) workspace_bytes += (int64_t)b.bytes;
        // (a small call splits the heat-map into more slabs: at most 191 / head_slabs crops take that split)
        const int64_t small_crops = std::min<int64_t>(max_batch, (191 + head_slabs) / head_slabs);
        const int64_t part = std::max((int64_t)max_batch * joints * head_slabs, small_crops * joints * head_slabs_small);
        workspace_bytes += part * 8;
        if (plan_only) {
            fill_problems();
            index_s2groups();
            // zero pages straight from the kernel, touched only where weights are written: calloc may hand back a recycled heap chunk and
            // clear all of it (over 100 MB per handle), which made sweeps over thousands of plan-only handles allocator-dependent
            blob = (char *)mmap(nullptr, (size_t)blob_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (blob == (char *)MAP_FAILED) blob = nullptr;
            return blob != nullptr;
        }
        if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return false;
        for (auto &b : buffers) {
            if (!hip_ok(hipMalloc((void **)&b.dev, b.bytes), "hipMalloc(activation)")) return false;
            if (!hip_ok(hipMemset(b.dev, 0, b.bytes), "hipMemset(activation)")) return false;
        }
        if (!hip_ok(hipMalloc((void **)&blob, (size_t)blob_bytes), "hipMalloc(weights)")) return false;
        if (!hip_ok(hipMemset(blob, 0, (size_t)blob_bytes), "hipMemset(weights)")) return false;
        if (!setup_groups() || !setup_dgroups() || !setup_s2groups()) return false;
        if (!hip_ok(hipMalloc((void **)&part_val, (size_t)part * 4), "hipMalloc(part_val)")) return false;
        if (!hip_ok(hipMalloc((void **)&part_idx, (size_t)part * 4), "hipMalloc(part_idx)")) return false;
        return hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }

    // every block walks ~`half_stages_per_block` half-slices so that blocks of all branches last alike
    int conv3_tiles_per_block(const ConvOp &cv) const {
        // (96-cout form: three stages of 18 MR MFMAs per slice, each about 0.86 of a (48, 3) half-stage)
        if (cv.n96) return std::max(1, (half_stages_per_block * 7) / (6 * 3 * cv.slices));
        const int t = half_stages_per_block / ((cv.ks == 48 ? 2 : 1) * cv.slices);
        return t < 1 ? 1 : t;
    }

    // A fusable BasicBlock runs fused (conv1's launch does both convolutions, conv2's launch skips it) when the call is
    // large enough; both launches decide by the same rule.
    bool bbf_active(const ConvOp &cv, int nb) const {
        return (nb * tensors[cv.out_t].hpwp + 511) / 512 >= bbf_min_tiles;
    }
    bool fused_now(const ConvOp &cv, int nb) const { return cv.fuse_with >= 0 && bbf_active(cv, nb); }
    bool skipped(const ConvOp &cv, int nb) const { return cv.fused_away && bbf_active(cv, nb); }

    // device-resident descriptors + block maps of the grouped conv launches
    int group_blocks(const Conv3Group &g, int nb, std::vector<int2> *out, bool reverse, bool all_short = false,
                     std::vector<int> *tile_px_out = nullptr) const {
        struct Ent {
            double key;
            int2 v;
            int bm;
        };
        std::vector<Ent> ents;
        // Block lengths follow the size of the launch: small batches get shorter blocks (at least ~2 per CU before
        // anything else), and long blocks are only worth it when there are many blocks per CU to begin with.
        // a few crops: even one tile per block leaves CUs idle -> 128-pixel tiles for the whole launch
        long one_per_block = 0;
        for (int ci : g.conv_idx) {
            const ConvOp &cv = convs[ci];
            if (skipped(cv, nb)) continue;
            const Tensor &to = tensors[cv.out_t];
            const int bmn = fused_now(cv, nb) ? 512 : conv3x3_lds_bm(cv.ks, cv.nr, to.wp);
            one_per_block += (long)((m_pixels(cv, to, nb) + bmn - 1) / bmn) * cv.ntiles;
        }
        const bool small = small_tiles && one_per_block < small_below;
        // a fused BasicBlock walks 512-pixel tiles through both convolutions (no small-tile mode): about three
        // ordinary 384-pixel tiles' worth of work each
        // fp32 form: a stage (one 16-channel slice of a 512-pixel tile) keeps a CU busy for ~8 us, so a one-tile block of the
        // 256-channel branch would run 16 of them back to back while the launch as a whole is ~20 stages of work per CU:
        // deep convolutions take 128-pixel tiles (the kernel picks the tile size per block) so that no block exceeds ~16
        // quarter-stages and the launch can balance
        // round 6: ... except that a SHORT convolution (one 48- or two 32-channel slices: two half-stages per tile, all of a small block's life
        // is its prologue) keeps its full tiles when 128-pixel tiles would put more than ~1.2 blocks per CU into the launch: 8 crops of
        // 384x288 made 443 + 196 blocks, and the 48-channel branch's 443 were half of the launch's CU time (profiles/round6_clip8_*)
        long small_blocks = 0;
        for (int ci : g.conv_idx) {
            const ConvOp &cv = convs[ci];
            if (skipped(cv, nb)) continue;
            small_blocks += (long)((m_pixels(cv, tensors[cv.out_t], nb) + 127) / 128) * cv.ntiles;
        }
        const bool keep_short_full = small && small_keep_above > 0 && small_blocks > small_keep_above;
        auto short_conv = [&](const ConvOp &cv) { return cv.ks != 16 && !cv.n96 && (cv.ks == 48 ? 2 : 1) * cv.slices <= 2; };
        auto small_conv = [&](const ConvOp &cv) {
            if (cv.ks == 16 && f32_small_slices > 0 && cv.slices >= f32_small_slices) return true;
            return small && !(keep_short_full && short_conv(cv));
        };
        auto tile_px = [&](const ConvOp &cv, const Tensor &to) {
            return fused_now(cv, nb) ? 512 : small_conv(cv) ? 128 : conv3x3_lds_bm(cv.ks, cv.nr, to.wp);
        };
        auto tiles_per_block = [&](const ConvOp &cv, int div) {
            return std::max(1, conv3_tiles_per_block(cv) / (fused_now(cv, nb) ? bbf_tpb_div : 1) / div);
        };
        auto count_blocks = [&](int div) {
            long total = 0;
            for (int ci : g.conv_idx) {
                const ConvOp &cv = convs[ci];
                if (skipped(cv, nb)) continue;
                const Tensor &to = tensors[cv.out_t];
                const int bm = tile_px(cv, to);
                const int mtiles = (int)((m_pixels(cv, to, nb) + bm - 1) / bm);
                const int tpb = tiles_per_block(cv, div);
                total += (long)((mtiles + tpb - 1) / tpb) * cv.ntiles;
            }
            return total;
        };
        int div = 1;
        while (div < 64 && count_blocks(div) < 512) div *= 2;
        int lf = all_short ? 1 : (int)std::min<long>(long_factor, count_blocks(div) / 768);
        if (lf < 1) lf = 1;
        for (size_t k = 0; k < g.conv_idx.size(); ++k) {
            const ConvOp &cv = convs[g.conv_idx[k]];
            if (skipped(cv, nb)) continue;
            const Tensor &to = tensors[cv.out_t];
            const int bm = tile_px(cv, to);
            const bool fused = fused_now(cv, nb);
            const int prob = fused ? g.fused_prob[k] : (int)k;
            const int mtiles = (int)((m_pixels(cv, to, nb) + bm - 1) / bm);
            // Blocks come in two lengths: long ones (fewer pipeline prologues -- a block's first loads have nothing to
            // hide behind) over the first `long_share` of the M tiles, short ones over the rest to fill the tail.
            const int tpb_short = tiles_per_block(cv, div);
            const int tpb_long = tpb_short * lf;
            const int long_tiles = ((int)(mtiles * long_share) / (8 * tpb_long)) * (8 * tpb_long);  // whole XCD rounds
            for (int phase = 0; phase < 2; ++phase) {
                const int tpb = phase == 0 ? tpb_long : tpb_short;
                const int first = phase == 0 ? 0 : long_tiles;
                const int count = phase == 0 ? long_tiles : mtiles - long_tiles;
                if (count <= 0) continue;
                const int mgroups = (count + tpb - 1) / tpb;
                const int total = mgroups * cv.ntiles;
                // XCD-aware order inside a problem: the hardware places block id b on XCD b % 8 (private L2 each).
                // Emit rounds of 8 M groups x all cout tiles with the M group varying fastest, so the cout tiles of one
                // M group are 8 ids apart = on the same XCD, and re-read its slab from that L2, not over the fabric.
                int seq = 0;
                for (int round = 0; round * 8 < mgroups; ++round)
                    for (int nt = 0; nt < cv.ntiles; ++nt)
                        for (int x = 0; x < 8; ++x) {
                            const int mg = round * 8 + x;
                            if (mg >= mgroups) continue;
                            const int i = seq++;
                            int tiles = count - mg * tpb;
                            if (tiles > tpb) tiles = tpb;
                            double key = (i + 0.5) / total;  // proportional interleave of the problems
                            if (block_order == 1)            // longest-processing-time first (estimated block cost)
                                key = -(fused ? 28000.0 + (tiles - 1) * bbf_slide_cost   // a fused block's later tiles slide (bbf_run)
                                        : (double)tiles * (cv.ks == 16 ? cv.slices * (double)bm * 36.0 + 2000.0   // fp32: 9 x 4 MR NRB MFMAs of 32 cycles per slice
                                                        : cv.n96      ? cv.slices * 3.0 * (bm == 512 ? 3900.0 : 3000.0) + (bm == 512 ? 7000.0 : 5000.0)
                                                                 : cv.slices * 2.0 * (bm == 512 ? 4300.0 : 3500.0) + (bm == 512 ? 5000.0 : 3000.0))) +
                                      1e-3 * key;
                            int mt0 = first + mg * tpb;
                            // every other launch walks the tensors backwards: a launch starts on what its producer
                            // wrote last, i.e. on the part most likely still in the Infinity Cache
                            if (reverse) mt0 = mtiles - mt0 - tiles;
                            ents.push_back({key, int2{prob | (nt << 8) | (tiles << 16), mt0 | (fused ? 1 << 29 : small_conv(cv) ? 1 << 30 : 0)}, bm});
                        }
            }
        }
        std::stable_sort(ents.begin(), ents.end(), [](const Ent &a, const Ent &b) { return a.key < b.key; });
        if (tile_px_out) {
            tile_px_out->resize(ents.size());
            for (size_t i = 0; i < ents.size(); ++i) (*tile_px_out)[i] = ents[i].bm;
        }
        if (out) {
            out->resize(ents.size());
            for (size_t i = 0; i < ents.size(); ++i) (*out)[i] = ents[i].v;
        }
        return (int)ents.size();
    }

    // the pixel grid a convolution iterates over: its output, or for a transposed-conv phase its input
    const Tensor &grid_of(const ConvOp &cv) const { return tensors[cv.up ? cv.in_t : cv.out_t]; }

    ConvArgs conv_args(const ConvOp &cv, int nb, bool rev) const {
        const Tensor &ti = tensors[cv.in_t], &to = grid_of(cv);
        ConvArgs a;
        a.in = row0(cv.in_t), a.out = row0(cv.out_t);
        a.w = blob + cv.w_off, a.bias = (const float *)(blob + cv.b_off);
        a.res = cv.res_t >= 0 ? row0(cv.res_t) : nullptr;
        a.cin = cv.cin, a.cout = cv.cout;
        a.in_wp = ti.wp, a.in_hpwp = ti.hpwp;
        a.out_h = to.h, a.out_w = to.w, a.out_wp = to.wp, a.out_hpwp = to.hpwp;
        a.m = nb * to.hpwp;
        a.ksize = cv.k, a.stride = cv.stride, a.relu = cv.relu, a.kchunks = cv.kchunks;
        a.rev = rev;
        a.pre_mode = pre_mode;
        a.wlds = direct_wlds && is16() ? 1 : 0;
        a.xlds = conv_xl(cv) ? 1 : 0;
        a.up = cv.up ? 1 : 0, a.up_a = cv.up ? (cv.up - 1) >> 1 : 0, a.up_b = cv.up ? (cv.up - 1) & 1 : 0;
        a.up_wp = tensors[cv.out_t].wp, a.up_hpwp = tensors[cv.out_t].hpwp;
        for (int t = 0; t < 4; ++t) {  // live tap t = ty*2 + tx of phase (a, b): dy = ty - 1 + a, dx = tx - 1 + b
            const int dy = (t >> 1) - 1 + a.up_a, dx = (t & 1) - 1 + a.up_b;
            a.taps[t] = cv.up ? dy * ti.wp + dx : 0;
        }
        return a;
    }

    // Block map of a grouped launch of the generic kernel.  Convolutions that read the same tensor with the same
    // window form a class; inside a class the map walks rounds of 8 M tiles and, per round, every (conv, cout tile)
    // of the class with the M tile varying fastest: block id b runs on XCD b % 8, so all readers of one input tile
    // are 8 ids apart = on one XCD, back to back, and the tile comes from HBM once.  Rounds are padded to 8 entries
    // (an out-of-range M tile returns at once) to keep that alignment.  Classes go out costliest first.
    int direct_group_blocks(const DirectGroup &g, int nb, std::vector<int2> *out, int mr = 4) const {
        struct Cls {
            int in_t, k, stride;
            std::vector<int> members;
            double cost = 0;
        };
        std::vector<Cls> cls;
        for (size_t k = 0; k < g.conv_idx.size(); ++k) {
            const ConvOp &cv = convs[g.conv_idx[k]];
            size_t ci = 0;
            for (; ci < cls.size(); ++ci)
                if (cls[ci].in_t == cv.in_t && cls[ci].k == cv.k && cls[ci].stride == cv.stride) break;
            if (ci == cls.size()) cls.push_back(Cls{cv.in_t, cv.k, cv.stride, {}, 0});
            cls[ci].members.push_back((int)k);
            cls[ci].cost += (double)grid_of(cv).hpwp * (cv.cout / (16 * g.nr)) * cv.kchunks;
        }
        std::stable_sort(cls.begin(), cls.end(), [](const Cls &a, const Cls &b) { return a.cost > b.cost; });
        int n = 0;
        if (out) out->clear();
        for (const Cls &cl : cls) {
            const int mtiles = (nb * grid_of(convs[g.conv_idx[cl.members[0]]]).hpwp + 64 * mr - 1) / (64 * mr);
            for (int round = 0; round * 8 < mtiles; ++round)
                for (int k : cl.members) {
                    const int ngroups = convs[g.conv_idx[k]].cout / (16 * g.nr);
                    for (int ng = 0; ng < ngroups; ++ng)
                        for (int x = 0; x < 8; ++x, ++n)
                            if (out) out->push_back(int2{k | (ng << 8), round * 8 + x});
                }
        }
        return n;
    }

    // pixels a convolution's launch enumerates: every flat row of the padded layout, or (compact 96-cout form) the real ones only
    int64_t m_pixels(const ConvOp &cv, const Tensor &to, int nb) const {
        return cv.compact ? (int64_t)nb * to.h * to.w : (int64_t)nb * to.hpwp;
    }
    // compact form: rows of the slab of a tile of `bm` real pixels = the longest run of flat rows such a tile spans (pad
    // columns and pad rows crossed included) + the halo above and below (wp + 1 rows each); tiles start at multiples of bm
    static int compact_slab_rows(int h, int w, int bm, int crops) {
        const int wp = w + 1, hpwp = (h + 1) * wp, hw = h * w;
        auto flat = [&](int64_t c) { const int64_t n = c / hw, r = c % hw; return n * hpwp + (r / w) * wp + r % w; };
        const int64_t m = (int64_t)crops * hw;
        int64_t span = 0;
        for (int64_t c0 = 0; c0 < m; c0 += bm) span = std::max(span, flat(std::min(c0 + bm, m) - 1) - flat(c0) + 1);
        return (int)span + 2 * wp + 2;
    }

    // 16-pixel fragments per wave of a grouped generic launch: shorter M tiles for small launches (fill the chip, shorten the
    // serial K loop per block)
    int direct_mr(const DirectGroup &g, int nb) const {
        int mr = 4;
        while (mr > 1 && direct_group_blocks(g, nb, nullptr, mr) < 512) mr >>= 1;
        return mr;
    }

    bool setup_dgroups() {
        for (auto &g : dgroups)
            // M tiles shrink (mr 4 -> 2 -> 1) only while a launch has fewer than 512 blocks: 4x that bounds every case
            if (!alloc_maps(g.maps, std::max<int64_t>(direct_group_blocks(g, max_batch, nullptr), 4 * 512 + 64 * (int64_t)g.conv_idx.size() * 8),
                            g.conv_idx.size()))
                return false;
        return true;
    }

    // ---- stride-2 slab kernel: descriptors (fixed at create) and block maps (per micro-batch size)
    size_t index_s2groups() {
        size_t n = 0;
        for (auto &g : s2groups) g.prob_first = (int)n, n += g.probs.size();
        if (stem_fuse) stemf.prob_first = (int)n, n += stemf.probs.size();   // (behind the launches of the pass: their numbering stays)
        return n;
    }
    long s2_tiles(const S2Group &g, int nb) const {
        long t = 0;
        for (auto &pr : g.probs) t += (long)nb * pr.tiles_per_image;
        return t;
    }
    // the slab kernel runs when the launch has a tile for every CU; smaller calls take the generic kernel (bit-identical)
    bool s2_active(const S2Group &g, int nb) const { return s2_tiles(g, nb) >= s2_min_tiles; }
    // Block map: every block walks a run of consecutive tiles of one problem (weights loaded once per block); run lengths are
    // chosen so that blocks of all problems cost about the same and the launch has ~s2_target_blocks of them, costliest first.
    int s2_blocks(const S2Group &g, int nb, std::vector<int2> *out) const {
        struct Ent {
            double key;
            int2 v;
        };
        std::vector<double> cost(g.probs.size());
        double total = 0;
        for (size_t k = 0; k < g.probs.size(); ++k) {
            const S2Group::Prob &pr = g.probs[k];
            const Tensor &to = tensors[convs[pr.parts[0].first].out_t];
            const int frags = (pr.rows * to.wp + 15) / 16;
            const int wm = std::max(1, 8 / (int)pr.parts.size());     // fewest waves sharing a part
            const int cin = convs[pr.parts[0].first].cin;
            cost[k] = (double)((frags + wm - 1) / wm) * ((9 * cin + 31) / 32) * s2_frags_per_part(cin) + 60;   // MFMAs of the busiest wave + per-tile overhead
            total += cost[k] * nb * pr.tiles_per_image;
        }
        const double per_block = total / s2_target_blocks;
        std::vector<Ent> ents;
        for (size_t k = 0; k < g.probs.size(); ++k) {
            const S2Group::Prob &pr = g.probs[k];
            const int tiles = nb * pr.tiles_per_image;
            int run = (int)(per_block / cost[k] + 0.5);
            run = run < 1 ? 1 : run > 64 ? 64 : run;
            // the fused stem: ONE problem of equal tiles -> exactly one block per CU (with runs capped at 64 a 256-crop call had 384
            // blocks for 256 CUs: half of the CUs ran two, the launch took 4/3 of its balanced time)
            if (&g == &stemf) run = (tiles + s2_target_blocks - 1) / s2_target_blocks;
            for (int t0 = 0; t0 < tiles; t0 += run) {
                const int cnt = tiles - t0 < run ? tiles - t0 : run;
                ents.push_back({-(cnt * cost[k]) + 1e-9 * t0, int2{(int)k | (cnt << 8), t0}});
            }
        }
        std::stable_sort(ents.begin(), ents.end(), [](const Ent &a, const Ent &b) { return a.key < b.key; });
        if (out) {
            out->resize(ents.size());
            for (size_t i = 0; i < ents.size(); ++i) (*out)[i] = ents[i].v;
        }
        return (int)ents.size();
    }

    // Eight waves over P parts: 8 / P waves per part (the first 8 % P parts one more), the waves of a part deal its pixel
    // fragments round-robin.  Wave w runs on SIMD w % 4: waves are placed so that the four SIMDs carry equal shares
    // (3 parts: 3 + 3 + 2 waves -> per-SIMD load 10 : 10 : 8 : 8 twelfths instead of 12 : 12 : 6 : 6 with 2 + 2 + 2).
    static void s2_wave_table(int nparts, unsigned char *part, unsigned char *f0, unsigned char *fs) {
        struct W {
            int p, i, m;
        };
        std::vector<W> ws;
        for (int p = 0; p < nparts; ++p) {
            const int m = std::max(1, 8 / nparts + (p < 8 % nparts ? 1 : 0));
            for (int i = 0; i < m && (int)ws.size() < 8; ++i) ws.push_back({p, i, m});
        }
        std::stable_sort(ws.begin(), ws.end(), [](const W &a, const W &b) { return a.m < b.m; });  // heaviest (fewest sharers) first
        double load[4] = {0, 0, 0, 0};
        bool used[8] = {};
        for (int w = 0; w < 8; ++w) part[w] = 0xff, f0[w] = 0, fs[w] = 1;
        for (const W &x : ws) {
            int best = -1;
            for (int w = 0; w < 8; ++w)
                if (!used[w] && (best < 0 || load[w & 3] < load[best & 3] - 1e-12)) best = w;
            used[best] = true;
            load[best & 3] += 1.0 / x.m;
            part[best] = (unsigned char)x.p, f0[best] = (unsigned char)x.i, fs[best] = (unsigned char)x.m;
        }
    }

    bool setup_s2groups() {
        const size_t nprob = index_s2groups();
        if (!nprob) return true;
        std::vector<S2Problem> hp(nprob);
        std::vector<S2Group *> all;
        for (auto &g : s2groups) all.push_back(&g);
        if (stem_fuse) all.push_back(&stemf);
        for (S2Group *gp : all) {
            S2Group &g = *gp;
            for (size_t k = 0; k < g.probs.size(); ++k) {
                const S2Group::Prob &pr = g.probs[k];
                const Tensor &ti = tensors[pr.in_t], &to = tensors[convs[pr.parts[0].first].out_t];
                S2Problem &q = hp[g.prob_first + k];
                memset(&q, 0, sizeof q);
                q.in = row0(pr.in_t), q.cin = ti.c, q.in_wp = ti.wp, q.in_hpwp = ti.hpwp;
                q.ho = to.h, q.wo = to.w, q.wop = to.wp, q.out_hpwp = to.hpwp;
                q.rows = pr.rows, q.tiles_per_image = pr.tiles_per_image;
                q.nparts = (int)pr.parts.size();
                s2_wave_table(q.nparts, q.wave_part, q.wave_f0, q.wave_fs);
                if (gp == &stemf)
                    // one output row = ceil(wop / 16) pixel fragments (5 at 288 columns) dealt to the 4 waves of a part: the wave
                    // with f0 = 0 takes two.  Part 1's waves start two further on, or both of those sit on SIMD 0 (waves w, w + 4)
                    for (int w = 0; w < 8; ++w)
                        if (q.wave_part[w] == 1 && q.wave_fs[w] == 4) q.wave_f0[w] = (unsigned char)((q.wave_f0[w] + 2) & 3);
                fast_div(to.wp, &q.magic_wop, &q.shift_wop);
                for (int i = 0; i < q.nparts; ++i) {
                    const ConvOp &cv = convs[pr.parts[i].first];
                    S2Part &pt = q.part[i];
                    const int nf = s2_frags_per_part(cv.cin);
                    pt.w = blob + cv.w2_off + (int64_t)pr.parts[i].second * ((9 * cv.cin + 31) / 32) * nf * 1024;
                    pt.bias = (const float *)(blob + cv.b_off);
                    pt.out = row0(cv.out_t);
                    pt.cout = cv.cout, pt.ch0 = pr.parts[i].second * 16 * nf, pt.relu = cv.relu;
                }
            }
            int64_t capacity = 64;
            for (auto &pr : g.probs) capacity += (int64_t)max_batch * pr.tiles_per_image;  // one tile per block bounds every split
            if (!alloc_maps(g.maps, capacity)) return false;
        }
        if (!hip_ok(hipMalloc((void **)&s2probs_dev, nprob * sizeof(S2Problem)), "hipMalloc(s2 problems)")) return false;
        return hip_ok(hipMemcpy(s2probs_dev, hp.data(), nprob * sizeof(S2Problem), hipMemcpyHostToDevice), "hipMemcpy(s2 problems)");
    }

    // ---- the block-map cache of a grouped launch (BlockMaps, ctx_types.h): every slot holds `capacity` blocks and, for the
    // generic kernel, `nargs` descriptors; all of it counts as workspace
    bool alloc_maps(BlockMaps &m, int64_t capacity, size_t nargs = 0) {
        m.capacity = capacity, m.nargs = nargs;
        for (MapSlot &sl : m.slot) {
            if (!hip_ok(hipMalloc((void **)&sl.dev, (size_t)capacity * sizeof(int2)), "hipMalloc(blockmap)")) return false;
            if (!hip_ok(hipHostMalloc((void **)&sl.pin, (size_t)capacity * sizeof(int2), hipHostMallocDefault), "hipHostMalloc(blockmap)"))
                return false;
            if (nargs) {
                if (!hip_ok(hipMalloc((void **)&sl.args_dev, nargs * sizeof(ConvArgs)), "hipMalloc(conv args)")) return false;
                if (!hip_ok(hipHostMalloc((void **)&sl.args_pin, nargs * sizeof(ConvArgs), hipHostMallocDefault), "hipHostMalloc(conv args)"))
                    return false;
            }
            if (!hip_ok(hipEventCreateWithFlags(&sl.landed, hipEventDisableTiming), "hipEventCreate")) return false;
            workspace_bytes += capacity * (int64_t)sizeof(int2) + (int64_t)(nargs * sizeof(ConvArgs));
        }
        return true;
    }
    void free_maps(BlockMaps &m) {
        for (MapSlot &sl : m.slot) {
            if (sl.dev) (void)hipFree(sl.dev);
            if (sl.pin) (void)hipHostFree(sl.pin);
            if (sl.args_dev) (void)hipFree(sl.args_dev);
            if (sl.args_pin) (void)hipHostFree(sl.args_pin);
            if (sl.landed) (void)hipEventDestroy(sl.landed);
            sl = MapSlot();
        }
    }
    // The slot holding the map of micro-batch size nb, ready for a launch on stream s (*out), or the error.  A miss runs
    // `build(slot, &scratch)` -- it fills the scratch (the generic kernel: also the slot's mr and args_pin) and returns the
    // block count -- and uploads on s: descriptors, then the map, then `landed`.  The slot takes its nb only after all of
    // that was queued: whatever fails on the way leaves it at nb == -1, and the next call builds again.
    template <class Build>
    hipError_t acquire_maps(BlockMaps &m, int nb, hipStream_t s, MapSlot **out, const Build &build) {
        bool hit;
        MapSlot *sl = *out = find_slot(m.slot, nb, &hit);
        hipError_t e = slot_ready(sl, hit, s);
        if (hit || e != hipSuccess) return e;
        sl->nblocks = build(sl, &m.host);
        if (sl->nblocks > m.capacity) return hipErrorInvalidValue;   // (ADVICE r3: never write past the slot)
        memcpy(sl->pin, m.host.data(), (size_t)sl->nblocks * sizeof(int2));
        if (m.nargs) e = hipMemcpyAsync(sl->args_dev, sl->args_pin, m.nargs * sizeof(ConvArgs), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sl->dev, sl->pin, (size_t)sl->nblocks * sizeof(int2), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(sl->landed, s);
        if (e != hipSuccess) return e;
        sl->nb = nb;
        ++map_builds;
        return hipSuccess;
    }
    // the slot holding the maps of micro-batch size nb, or the least recently used one to rebuild (*hit = false); a
    // slot about to be rebuilt has had its previous upload waited for, so its pinned image may be rewritten
    MapSlot *find_slot(MapSlot (&slots)[kMapSlots], int nb, bool *hit) {
        MapSlot *lru = &slots[0];
        for (MapSlot &sl : slots) {
            if (sl.nb == nb) {
                sl.stamp = ++map_clock;
                *hit = true;
                return &sl;
            }
            if (sl.stamp < lru->stamp) lru = &sl;
        }
        *hit = false;
        if (lru->nb >= 0) (void)hipEventSynchronize(lru->landed);
        lru->nb = -1;
        lru->stamp = ++map_clock;
        return lru;
    }

    // a cached map was uploaded on sl->up_stream; a launch on another stream has to see that upload (ADVICE r2: callers that
    // alternate streams on one handle -- predict_stream, user code under torch.cuda.stream)
    hipError_t slot_ready(MapSlot *sl, bool hit, hipStream_t s) {
        if (hit && sl->up_stream != s) return hipStreamWaitEvent(s, sl->landed, 0);
        if (!hit) sl->up_stream = s;
        return hipSuccess;
    }

    // descriptor numbering of the grouped launches (host only; plan-only handles need it for hrn_plan_block_map)
    size_t index_groups() {
        size_t nprob = 0;
        for (auto &g : groups) {
            g.prob_first = (int)nprob;
            nprob += g.conv_idx.size();
            g.fused_prob.assign(g.conv_idx.size(), -1);
            int extra = (int)g.conv_idx.size();
            for (size_t k = 0; k < g.conv_idx.size(); ++k)
                if (convs[g.conv_idx[k]].fuse_with >= 0) g.fused_prob[k] = extra++, ++nprob;  // a second descriptor: the fused form
        }
        return nprob;
    }

    // the descriptors of the grouped launches on the host (plan-only handles: the same, with the pointers of an unallocated
    // workspace -- the plan queries read the geometry only)
    size_t fill_problems() {
        const size_t nprob = index_groups();
        probs_host.assign(nprob, Conv3Problem{});
        std::vector<Conv3Problem> &hp = probs_host;
        for (auto &g : groups) {
            g.max_wp = 0;
            for (size_t k = 0; k < g.conv_idx.size(); ++k) {
                const ConvOp &cv = convs[g.conv_idx[k]];
                const Tensor &to = tensors[cv.out_t];
                Conv3Problem &q = hp[g.prob_first + k];
                q.in = row0(cv.in_t), q.out = row0(cv.out_t);
                q.w = blob + cv.w_off, q.bias = (const float *)(blob + cv.b_off);
                q.res = cv.res_t >= 0 ? row0(cv.res_t) : nullptr;
                q.cin = cv.cin, q.cout = cv.cout, q.h = to.h, q.wd = to.w, q.wp = to.wp, q.hpwp = to.hpwp;
                q.relu = cv.relu, q.slices = cv.slices, q.ntiles = cv.ntiles;
                q.w2 = nullptr, q.bias2 = nullptr;
                q.n96 = cv.n96 ? 1 : 0;
                q.compact = cv.compact ? 1 : 0, q.hw = to.h * to.w;
                q.slab_rows = q.slab_rows_small = 0;
                if (cv.compact) {
                    fast_div(q.hw, &q.magic_hw, &q.shift_hw);
                    fast_div(to.w, &q.magic_w, &q.shift_w);
                    q.slab_rows = compact_slab_rows(to.h, to.w, 512, max_batch), q.slab_rows_small = compact_slab_rows(to.h, to.w, 128, max_batch);
                }
                q.tiles_per_block = conv3_tiles_per_block(cv);
                q.bm = conv3x3_lds_bm(cv.ks, cv.nr, to.wp);
                fast_div(to.hpwp, &q.magic_hpwp, &q.shift_hpwp);
                fast_div(to.wp, &q.magic_wp, &q.shift_wp);
                if (to.wp > g.max_wp) g.max_wp = to.wp;
                if (cv.fuse_with >= 0) {  // the whole BasicBlock: in = x (also the residual), out = the block's output
                    const ConvOp &c2 = convs[cv.fuse_with];
                    Conv3Problem &f = hp[g.prob_first + g.fused_prob[k]];
                    f = q;
                    f.out = row0(c2.out_t), f.relu = c2.relu, f.res = nullptr;
                    f.w2 = blob + c2.w_off, f.bias2 = (const float *)(blob + c2.b_off);
                }
            }
        }
        return nprob;
    }

    bool setup_groups() {
        const size_t nprob = fill_problems();
        if (!nprob) return true;
        std::vector<Conv3Problem> &hp = probs_host;
        for (auto &g : groups) {
            int64_t capacity = 64 + 4 * (int64_t)std::max(small_below, 256) + 1024;  // one M tile per block = most blocks any split can produce (+ the small-tile mode)
            for (int ci : g.conv_idx) {
                const ConvOp &cv = convs[ci];
                const Tensor &to = tensors[cv.out_t];
                // (128-pixel tiles whenever a knob may ask for them: HRN_F32_SMALL_SLICES -- ADVICE r3)
                const int bm = f32_small_slices > 0 ? 128 : conv3x3_lds_bm(cv.ks, cv.nr, to.wp);
                capacity += (int64_t)((max_batch * to.hpwp + bm - 1) / bm) * cv.ntiles;   // (compact convolutions have fewer)
            }
            if (!alloc_maps(g.maps, capacity)) return false;
        }
        if (!hip_ok(hipMalloc((void **)&probs_dev, nprob * sizeof(Conv3Problem)), "hipMalloc(problems)")) return false;
        return hip_ok(hipMemcpy(probs_dev, hp.data(), nprob * sizeof(Conv3Problem), hipMemcpyHostToDevice),
                      "hipMemcpy(problems)");
    }

    void free_all() {
        if (plan_only) {
            if (blob) (void)munmap(blob, (size_t)blob_bytes);
        } else {
            (void)hipSetDevice(device);
            for (auto &b : buffers)
                if (b.dev) (void)hipFree(b.dev);
            if (blob) (void)hipFree(blob);
            if (scratch_hm) (void)hipFree(scratch_hm);
            free_scratch();
            if (part_val) (void)hipFree(part_val);
            if (part_idx) (void)hipFree(part_idx);
            if (probs_dev) (void)hipFree(probs_dev);
            if (s2probs_dev) (void)hipFree(s2probs_dev);
            for (auto &g : s2groups) free_maps(g.maps);
            free_maps(stemf.maps);
            for (auto &g : groups) free_maps(g.maps);
            for (auto &g : dgroups) free_maps(g.maps);
        }
        blob = nullptr;
    }

    char *row0(int t) const {
        const Tensor &tt = tensors[t];
        const Buffer &b = buffers[tt.buf];
        return b.dev ? b.dev + b.lead_rows * tt.c * esize : nullptr;
    }

