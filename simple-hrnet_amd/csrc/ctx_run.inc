// struct hrn_ctx, part: execution -- one pass = the launch list on a stream; argument checks.
// Included INSIDE the struct body by hrnet_mi355.cpp (member functions defined in place; one type, split by concern:
// ctx_plan / ctx_memory / ctx_weights / ctx_run).
    // ---------------------------------------------------------------- execution
    struct Timing {
        std::vector<hipEvent_t> ev;  // ops.size()+1 events
    };

    // every other launch walks its tensors backwards: it starts on what its producer wrote last, i.e. on the
    // part most likely still in the Infinity Cache (256 MB; a 256-crop tensor is up to 0.9 GB)
    bool walks_back(size_t oi) const { return alternate && (oi & 1); }

    bool run_pass(const float *images, int nb, const void *boxes, int box_dtype, float *pts, float *heatmaps,
                  hipStream_t s, Timing *tm, int flip = 0, const TapReq *tap = nullptr, int refine = RF_NONE) {
        if (tm && !hip_ok(hipEventRecord(tm->ev[0], s), "hipEventRecord")) return false;
        // the fused stem writes conv2's output only: a call that taps "stem" (ops[0]'s tensor) takes the two launches
        const bool fused_stem = stem_fuse && !(tap && tap->op == 0);
        for (size_t oi = 0; oi < ops.size(); ++oi) {
            const bool rev = walks_back(oi);
            hipError_t e = hipSuccess;
            if (fused_stem && oi == 0)
                e = exec_stem_fused(images, nb, s, flip);
            else if (!(fused_stem && (int)oi == stem_conv2_op))
                e = exec_op(ops[oi], rev, images, nb, boxes, box_dtype, pts, heatmaps, s, flip, refine);
            if (!hip_ok(e, "kernel launch")) return false;
            if (tap && tap->op == (int)oi) {  // debug tap: the tensor this launch completed, as (ncrops, C, H, W) fp32
                const Tensor &t = tensors[tap->tensor];
                TapArgs a;
                a.in = row0(tap->tensor), a.dst = tap->dst;
                a.c = t.c, a.h = t.h, a.w = t.w, a.wp = t.wp, a.hpwp = t.hpwp;
                a.crop0 = tap->crop0, a.ncrops = tap->ncrops, a.crop_step = tap->crop_step;
                if (!hip_ok(launch_tap(dtype, a, s), "tap launch")) return false;
            }
            if (tm && !hip_ok(hipEventRecord(tm->ev[oi + 1], s), "hipEventRecord")) return false;
        }
        return true;
    }

    // conv1's arguments (StemArgs and Stem7Args carry the same fields): `out` = its tensor, `w` = the fp32 weights, `wp` = their
    // MFMA image (nullptr: the kernel takes `w`)
    template <class Args>
    Args stem_args(const float *images, int nb, int flip, void *out, const float *w, const void *wp) const {
        const Tensor &t = tensors[stem_out_t];
        Args a;
        a.images = images, a.out = out;
        a.w = w, a.bias = (const float *)(blob + stem_b_off), a.wp = wp;
        a.n = nb, a.H = H, a.W = W;
        a.out_h = t.h, a.out_w = t.w, a.out_wp = t.wp, a.out_hpwp = t.hpwp;
        a.flip = flip;
        return a;
    }
    // ... of conv1's own launch
    template <class Args>
    Args stem_args(const float *images, int nb, int flip) const {
        return stem_args<Args>(images, nb, flip, row0(stem_out_t), (const float *)(blob + stem_w_off),
                               (is16() && !disable_stem_mfma) ? (const void *)(blob + stem_wp_off) : nullptr);
    }

    hipError_t exec_stem_fused(const float *images, int nb, hipStream_t s, int flip) {
        S2Group &g = stemf;
        MapSlot *sl = nullptr;
        hipError_t e = acquire_maps(g.maps, nb, s, &sl, [&](MapSlot *, std::vector<int2> *map) { return s2_blocks(g, nb, map); });
        if (e != hipSuccess) return e;
        // (conv1 writes no tensor and reads no fp32 weights here: always the MFMA image)
        const StemArgs a = stem_args<StemArgs>(images, nb, flip, nullptr, nullptr, (const void *)(blob + stem_wp_off));
        return launch_stem_fused(dtype, s2probs_dev + g.prob_first, sl->dev, sl->nblocks, a, s);
    }

    hipError_t exec_op(const Op &op, bool rev, const float *images, int nb, const void *boxes, int box_dtype, float *pts,
                       float *heatmaps, hipStream_t s, int flip, int refine) {
        hipError_t e = hipSuccess;
        MapSlot *sl = nullptr;
        switch (op.kind) {
        case OP_STEM:
            e = launch_stem(dtype, stem_args<StemArgs>(images, nb, flip), s);
            break;
        case OP_STEM7:
            e = launch_stem7(dtype, stem_args<Stem7Args>(images, nb, flip), s);
            break;
        case OP_MAXPOOL: {
            const Tensor &ti = tensors[pool_in_t], &to = tensors[pool_out_t];
            PoolArgs a;
            a.in = row0(pool_in_t), a.out = row0(pool_out_t);
            a.c = to.c, a.n = nb, a.in_wp = ti.wp, a.in_hpwp = ti.hpwp;
            a.out_h = to.h, a.out_w = to.w, a.out_wp = to.wp, a.out_hpwp = to.hpwp;
            e = launch_maxpool(dtype, a, s);
            break;
        }
        case OP_CONV: {
            const ConvOp &cv = convs[op.idx];
            const ConvArgs a = conv_args(cv, nb, rev);
            e = launch_conv(dtype, a, cv.nr, s);
            break;
        }
        case OP_CONV3_GROUP: {   // block map depends on the micro-batch size: built once per size (kMapSlots sizes kept)
            Conv3Group &g = groups[op.idx];
            e = acquire_maps(g.maps, nb, s, &sl, [&](MapSlot *, std::vector<int2> *map) { return group_blocks(g, nb, map, rev); });
            if (e != hipSuccess) break;
            e = launch_conv3x3_lds(dtype, probs_dev + g.prob_first, sl->dev, sl->nblocks, nb, convs[g.conv_idx[0]].ks, convs[g.conv_idx[0]].nr, s);
            break;
        }
        case OP_CONV_GROUP: {   // descriptors (row counts), M tile and block map depend on the micro-batch size
            DirectGroup &g = dgroups[op.idx];
            e = acquire_maps(g.maps, nb, s, &sl, [&](MapSlot *slot, std::vector<int2> *map) {
                for (size_t k = 0; k < g.conv_idx.size(); ++k) slot->args_pin[k] = conv_args(convs[g.conv_idx[k]], nb, rev);
                slot->mr = direct_mr(g, nb);
                return direct_group_blocks(g, nb, map, slot->mr);
            });
            if (e != hipSuccess) break;
            int wl = direct_wlds && is16() ? 1 : 0;   // 2: a member takes the XL form (its LDS layout is the larger one)
            if (wl)
                for (int ci : g.conv_idx)
                    if (conv_xl(convs[ci])) wl = 2;
            e = launch_conv_group(dtype, sl->args_dev, sl->dev, sl->nblocks, g.nr, sl->mr, wl, s);
            break;
        }
        case OP_S2_GROUP: {
            S2Group &g = s2groups[op.idx];
            if (!s2_active(g, nb)) {  // too few tiles for the slab kernel: the same convolutions on the generic kernel
                for (const Op &f : g.fallback) {
                    e = exec_op(f, rev, images, nb, boxes, box_dtype, pts, heatmaps, s, flip, refine);
                    if (e != hipSuccess) break;
                }
                break;
            }
            e = acquire_maps(g.maps, nb, s, &sl, [&](MapSlot *, std::vector<int2> *map) { return s2_blocks(g, nb, map); });
            if (e != hipSuccess) break;
            e = launch_conv_s2(dtype, s2probs_dev + g.prob_first, sl->dev, sl->nblocks, s);
            break;
        }
        case OP_CHAIN: {
            const Chain &ch = chains[op.idx];
            const ConvOp &c3 = convs[ch.conv3];
            const Tensor &to = tensors[c3.out_t];
            ChainArgs a;
            a.in = row0(c3.in_t), a.res = row0(c3.res_t), a.out_y = row0(c3.out_t);
            a.w3 = blob + c3.w_off, a.b3 = (const float *)(blob + c3.b_off);
            a.out_t = nullptr, a.w1 = nullptr, a.b1 = nullptr;
            if (ch.conv1 >= 0) {
                const ConvOp &c1 = convs[ch.conv1];
                a.out_t = row0(c1.out_t), a.w1 = blob + c1.w_off, a.b1 = (const float *)(blob + c1.b_off);
            }
            a.in3 = nullptr, a.w2 = nullptr, a.b2 = nullptr;
            if (ch.conv2 >= 0) {   // the 3x3 in front: conv3's input tensor is never written, conv2's input is read instead
                const ConvOp &c2 = convs[ch.conv2];
                a.in3 = row0(c2.in_t), a.w2 = blob + c2.w_off, a.b2 = (const float *)(blob + c2.b_off);
                a.in = nullptr;
            }
            a.x = nullptr, a.wds = nullptr, a.bds = nullptr;
            if (ch.ds >= 0) {
                const ConvOp &cd = convs[ch.ds];
                a.x = row0(cd.in_t), a.wds = blob + cd.w_off, a.bds = (const float *)(blob + cd.b_off);
                a.res = nullptr;
            }
            a.m = nb * to.hpwp, a.h = to.h, a.w = to.w, a.wp = to.wp, a.hpwp = to.hpwp, a.rev = rev, a.max_blocks = chain_blocks;
            e = launch_bottleneck_chain(dtype, a, s);
            break;
        }
        case OP_FUSE: {
            FuseGroupArgs ga;
            ga.nf = fuses[op.idx].group;
            for (int k = 0; k < ga.nf; ++k) {
                const FuseOp &f = fuses[op.idx + k];
                const Tensor &to = tensors[f.out_t];
                FuseArgs &a = ga.f[k];
                a.nterms = f.nterms;
                for (int i = 0; i < f.nterms; ++i) {
                    const Tensor &tt = tensors[f.term_t[i]];
                    a.t[i].ptr = row0(f.term_t[i]), a.t[i].shift = f.shift[i];
                    a.t[i].wp = tt.wp, a.t[i].hpwp = tt.hpwp;
                }
                for (int i = f.nterms; i < 4; ++i) a.t[i] = FuseTerm{nullptr, 0, 0, 0};
                a.out = row0(f.out_t), a.c = to.c, a.h = to.h, a.w = to.w, a.wp = to.wp, a.hpwp = to.hpwp;
                a.m = nb * to.hpwp, a.rev = rev;
            }
            e = ga.nf == 1 ? launch_fuse(dtype, ga.f[0], s) : launch_fuse_group(dtype, ga, s);
            break;
        }
        case OP_HEAD: {
            const Tensor &t = tensors[head_in_t];
            HeadArgs a;
            a.in = row0(head_in_t);
            a.wgt = (const float *)(blob + head_w_off), a.bias = (const float *)(blob + head_b_off);
            a.wimg = (is16() && !disable_head_mfma) ? (const void *)(blob + head_wp_off) : nullptr;
            a.heatmaps = heatmaps, a.part_val = part_val, a.part_idx = part_idx;
            a.n = nb, a.c = t.c, a.joints = joints, a.h = t.h, a.w = t.w, a.wp = t.wp, a.hpwp = t.hpwp;
            a.slabs = head_slabs_for(nb), a.slab_px = head_px_for(nb);
            e = launch_head(dtype, a, s);
            break;
        }
        case OP_DECODE: {   // decode_kernel<refine>: a sub-pixel mode reads the heat-maps the head just wrote (hrn_forward_refined)
            if (!pts) break;
            const Tensor &t = tensors[head_in_t];
            DecodeArgs a{};
            a.part_val = part_val, a.part_idx = part_idx, a.heatmaps = heatmaps, a.boxes = boxes;
            a.box_is_float = box_dtype == HRN_BOX_F32, a.pts = pts;
            a.n = nb, a.joints = joints, a.h = t.h, a.w = t.w, a.slabs = head_slabs_for(nb), a.mode = refine;
            e = launch_decode(a, s);
            break;
        }
    }
        return e;
    }

    bool check_forward_args(const void *images, int n, const void *boxes, float *pts, float *heatmaps, bool outputs_optional = false) {
        if (refuse_plan_only()) return false;
        if (!weights_loaded) {
            err = "weights not loaded (call hrn_load_weights or hrn_adopt_weights)";
            return false;
        }
        if (n < 0 || (n > 0 && !images)) {
            err = "bad images / n";
            return false;
        }
        if (!pts && !heatmaps && !outputs_optional) {
            err = "both pts and heatmaps are NULL";
            return false;
        }
        if (pts && !boxes && n > 0) {
            err = "pts requested without boxes";
            return false;
        }
        return true;
    }
