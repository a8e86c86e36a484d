// struct hrn_ctx, part: the graph compiler -- tensors, convolutions, launch groups, the static launch list (models_/hrnet.py:75-189, models_/poseresnet.py:16-122).
// Included INSIDE the struct body by hrnet_mi355.cpp (member functions defined in place; one type, split by concern:
// ctx_plan / ctx_memory / ctx_weights / ctx_run).
    // ---------------------------------------------------------------- planning
    // INVARIANT of the workspace (every 3x3 convolution's zero padding rests on it; ADVICE r3): the pad column / pad row of every
    // image and the guard rows of a buffer hold ZEROS at all times.  Buffers are zeroed once when they are allocated and are only
    // ever reused by tensors of the SAME (channels, height, width) -- the free list below is keyed by geometry -- so pad positions
    // stay pad positions; every kernel that writes an activation either stores zeros at the pad positions it covers (the stride-1
    // kernels, the generic kernel, the fuse / stem / pool kernels) or never touches them (the stride-2 slab kernel, conv_s2.hip,
    // writes real output rows only: the pad row below the last one keeps the zeros it was allocated with).  A kernel that left
    // anything else in a pad position would silently change every downstream 3x3 convolution.
    int new_tensor(int ch, int h, int w) {
        Tensor t;
        t.c = ch, t.h = h, t.w = w, t.wp = w + 1, t.hp = h + 1, t.hpwp = t.wp * t.hp;
        for (size_t i = 0; i < buffers.size(); ++i)
            if (!buffers[i].in_use && buffers[i].c == ch && buffers[i].h == h && buffers[i].w == w) {
                t.buf = (int)i;
                break;
            }
        if (t.buf < 0) {
            Buffer b;
            b.c = ch, b.h = h, b.w = w;
            b.lead_rows = (size_t)t.wp + 1;
            // image rows + bottom halo + one conv block of overrun (masked lanes still form addresses)
            b.rows = b.lead_rows + (size_t)max_batch * t.hpwp + t.wp + 1 + kConvBlockRows;
            b.bytes = (size_t)align_up((int64_t)(b.rows * ch * esize), 256);
            buffers.push_back(b);
            t.buf = (int)buffers.size() - 1;
        }
        buffers[t.buf].in_use = true;
        tensors.push_back(t);
        return (int)tensors.size() - 1;
    }
    void release(int t) { buffers[tensors[t].buf].in_use = false; }

    int default_nr(int cout, int stride) const {
        int nr = (cout % 64 == 0) ? 4 : (cout % 48 == 0) ? 3 : 2;
        if (is16() && stride == 2 && cout % 96 == 0 && direct_nr6) nr = 6;  // halves the A gathers per MFMA
        return nr;
    }
    // widest cout tile every member of a set of sibling convolutions can use
    int common_nr(const std::vector<int> &couts, int stride) const {
        bool all64 = true, all48 = true, all96 = true;
        for (int co : couts) all64 &= co % 64 == 0, all48 &= co % 48 == 0, all96 &= co % 96 == 0;
        if (is16() && stride == 2 && all96 && direct_nr6) return 6;
        return all64 ? 4 : all48 ? 3 : 2;
    }

    // output rows per tile of the stride-2 slab kernel: as many as one slab buffer holds ((2R + 1) virtual input rows of
    // 2 * wop slots of 96 bytes)
    static int s2_rows(int wop, int ho, int cin) {
        // R output rows need R row pairs (s2_pair_pitch slots each, pad included) + the one virtual row above the next pair
        const int r = (s2_slot_capacity(cin) - 2 * wop) / s2_pair_pitch(wop);
        return r > ho ? ho : (r < 0 ? 0 : r);
    }

    int add_conv(const std::string &conv, const std::string &bn, int in_t, int cout, int k, int stride, int relu,
                 int res_t = -1, bool emit = true, int nr_override = 0, int up = 0, int up_out_t = -1, bool force_generic = false) {
        const Tensor ti = tensors[in_t];  // by value: new_tensor() below may reallocate `tensors`
        ConvOp op;
        op.conv = conv, op.bn = bn, op.in_t = in_t, op.res_t = res_t;
        op.cin = ti.c, op.cout = cout, op.k = k, op.stride = stride, op.relu = relu;
        const int oh = ti.h / stride, ow = ti.w / stride;
        op.up = up;
        op.out_t = up ? up_out_t : new_tensor(cout, oh, ow);
        const int kc = is16() ? 32 : 16;
        const int K = k * k * op.cin;
        op.kchunks = (K + kc - 1) / kc;
        op.kpad = op.kchunks * kc;
        op.nr = nr_override ? nr_override : default_nr(cout, stride);
        op.flops = 2.0 * cout * (double)K * oh * ow;
        // pipelined LDS kernel (conv3x3_lds.hip): KS = 48 / 48-cout tiles for the HRNet-W48 branch widths, KS = 32 with
        // 64-, 48- or 32-cout tiles for everything else whose channel counts are multiples of 32
        int lds_ks = 0, lds_nrb = 0;
        if (is16() && k == 3 && stride == 1 && !disable_lds && !up && !force_generic) {
            // widths that are multiples of 96 (the 96 / 192 / 384-channel branches of W48): 96 couts per block, 32-channel slices.
            // At EVERY batch size (its K order differs from the other forms'); its address arithmetic is 32-bit: tensors < 4 GB.
            const int64_t out_bytes = ((int64_t)max_batch * (oh + 1) * (ow + 1) + 2 * (ow + 2) + 512) * std::max(op.cin, cout) * 2;
            if (!disable_n96 && op.cin % 32 == 0 && cout % 96 == 0 && conv3x3_lds_bm(32, 6, ow + 1) > 0 && out_bytes < (int64_t(1) << 32))
                lds_ks = 32, lds_nrb = 6, op.n96 = true;
            else if (op.cin % 48 == 0 && cout % 48 == 0)
                lds_ks = 48, lds_nrb = 3;
            else if (op.cin % 32 == 0 && !disable_lds32)
                lds_ks = 32, lds_nrb = cout % 64 == 0 ? 4 : cout % 48 == 0 ? 3 : cout % 32 == 0 ? 2 : 0;
            if (lds_nrb && conv3x3_lds_bm(lds_ks, lds_nrb, ow + 1) == 0) lds_nrb = 0;
            // the 96-cout form over real pixels only where the padding of the flat layout is a large enough share of them (24x18: 9 %, 12x9: 17 %;
            // 48x36: 4.7 % -- less than the per-fragment addressing costs) and a tile's slab still fits its LDS buffer
            if (op.n96 && lds_nrb == 6 && !disable_compact && conv3x3_lds_bm(32, 6, ow + 1) == 512 &&
                1.0 - (double)(oh * ow) / ((oh + 1) * (ow + 1)) >= compact_min_pad &&
                // (the last LDS-DMA piece of a slab is written in whole 64-unit = 16-row chunks: the rows rounded up to 16 must fit)
                (compact_slab_rows(oh, ow, 512, max_batch) + 15) / 16 * 16 <= conv3x3_n96_max_rows() && (int64_t)max_batch * oh * ow < (int64_t(1) << 27))
                op.compact = true;
        }
        if (lds_nrb) {
            op.algo = 1, op.ks = lds_ks, op.nr = lds_nrb;
            op.slices = op.cin / lds_ks, op.ntiles = cout / (16 * lds_nrb), op.nch = (9 * lds_ks + 31) / 32;
            op.kpad = op.nch * 32 * op.slices;
        }
        // fp32 (the parity mode): the LDS-staged fp32 kernel (conv3x3_f32.hip) -- 16-channel slices, one K chunk of 16 per tap,
        // 48- or 32-cout tiles; everything whose channel counts allow it, at every batch size (its K order is its own)
        if (dtype == HRN_F32 && k == 3 && stride == 1 && !up && !disable_lds && !disable_f32lds && op.cin % 16 == 0 &&
            (cout % 48 == 0 || cout % 32 == 0) && conv3x3_lds_bm(16, cout % 48 == 0 ? 3 : 2, ow + 1) > 0) {
            op.algo = 1, op.ks = 16, op.nr = cout % 48 == 0 ? 3 : 2;
            op.slices = op.cin / 16, op.ntiles = cout / (16 * op.nr), op.nch = 9;
            op.kpad = 9 * 16 * op.slices;
        }
        if (is16() && k == 3 && stride == 2 && (op.cin == 48 || op.cin == 32 || op.cin == 64) &&   // (cin = 96 does not fit the registers: conv_s2.hip)
            cout % (16 * s2_frags_per_part(op.cin)) == 0 && !up && !disable_s2 && op.algo == 0 &&
            // at least two output rows per tile (or the whole image): with one, half of every slab is halo (three input rows
            // for one output row -- the 64 -> 64 stem conv of a 384x288 net) and the kernel moves 1.5x the tensor
            (s2_rows(ow + 1, oh, op.cin) >= 2 || s2_rows(ow + 1, oh, op.cin) == oh))
            op.s2 = true;
        convs.push_back(op);
        if (emit) emit_convs({(int)convs.size() - 1});
        return op.out_t;
    }

    // the (48, 3) and the (32, 6) form live in one kernel (conv3x3_lds_kernel<48, 3>) and share launches
    static int c3_family(const ConvOp &cv) { return ((cv.ks == 48 && cv.nr == 3) || cv.n96) ? 0 : cv.ks * 16 + cv.nr; }

    // emit a set of mutually independent convolutions: one grouped launch when all of them run on the
    // LDS-staged kernel, individual launches otherwise
    // convolutions on the generic kernel -> launches appended to `dst`: one grouped launch per cout-tile width
    void emit_direct(const std::vector<int> &idx, std::vector<Op> &dst) {
        std::vector<std::vector<int>> dsets;
        for (int i : idx) {
            if (disable_dgroup) {
                dst.push_back({OP_CONV, i});
                continue;
            }
            bool placed = false;
            for (auto &set : dsets)
                if (convs[set[0]].nr == convs[i].nr && set.size() < 255) {
                    set.push_back(i);
                    placed = true;
                    break;
                }
            if (!placed) dsets.push_back({i});
        }
        for (auto &set : dsets) {
            if (set.size() == 1) {
                dst.push_back({OP_CONV, set[0]});
                continue;
            }
            DirectGroup g;
            g.conv_idx = set, g.nr = convs[set[0]].nr;
            dgroups.push_back(g);
            dst.push_back({OP_CONV_GROUP, (int)dgroups.size() - 1});
        }
    }

    void emit_convs(const std::vector<int> &idx) {
        std::vector<int> lds, direct, s2;
        for (int i : idx) {
            if (convs[i].algo == 1)
                lds.push_back(i);
            else if (convs[i].s2)
                s2.push_back(i);
            else
                direct.push_back(i);
        }
        emit_direct(direct, ops);
        if (!s2.empty()) {
            // stride-2 slab kernel: one problem per input tensor (at most 8 parts of 48 couts each), all of them one launch
            S2Group g;
            g.conv_idx = s2;
            for (int i : s2) {
                const ConvOp &cv = convs[i];
                for (int t = 0; t < cv.cout / (16 * s2_frags_per_part(cv.cin)); ++t) {
                    S2Group::Prob *pr = nullptr;
                    for (auto &q : g.probs)
                        if (q.in_t == cv.in_t && (int)q.parts.size() < kS2MaxParts) pr = &q;
                    if (!pr) {
                        g.probs.push_back(S2Group::Prob());
                        pr = &g.probs.back();
                        pr->in_t = cv.in_t;
                        const Tensor &to = tensors[cv.out_t];
                        pr->rows = s2_rows(to.wp, to.h, cv.cin);
                        pr->tiles_per_image = (to.h + pr->rows - 1) / pr->rows;
                    }
                    pr->parts.push_back({i, t});
                }
            }
            emit_direct(s2, g.fallback);
            s2groups.push_back(g);
            ops.push_back({OP_S2_GROUP, (int)s2groups.size() - 1});
        }
        if (lds.empty()) return;
        std::vector<std::vector<int>> sets;  // one launch per (KS, NRB) configuration
        for (int i : lds) {
            bool placed = false;
            if (!disable_group)
                for (auto &set : sets)
                    if (c3_family(convs[set[0]]) == c3_family(convs[i])) {
                        set.push_back(i);
                        placed = true;
                        break;
                    }
            if (!placed) sets.push_back({i});
        }
        for (auto &set : sets) {
            Conv3Group g;
            g.conv_idx = set;
            groups.push_back(g);
            ops.push_back({OP_CONV3_GROUP, (int)groups.size() - 1});
        }
    }

    int add_fuse(const std::vector<int> &terms, const std::vector<int> &shifts, const std::string &name) {
        FuseOp f;
        f.name = name;
        f.nterms = (int)terms.size();
        for (int i = 0; i < f.nterms; ++i) f.term_t[i] = terms[i], f.shift[i] = shifts[i];
        const Tensor &t0 = tensors[terms[0]];
        // output geometry = geometry of a shift-0 term
        int ref = -1;
        for (int i = 0; i < f.nterms; ++i)
            if (shifts[i] == 0) ref = terms[i];
        const Tensor &tr = tensors[ref >= 0 ? ref : terms[0]];
        (void)t0;
        f.out_t = new_tensor(tr.c, tr.h, tr.w);
        fuses.push_back(f);
        return f.out_t;
    }

    // StageModule, hrnet.py:7-71
    void add_stage(const std::string &name, std::vector<int> &xs, int nout) {
        const int nb = (int)xs.size();
        char buf[160];
        // BasicBlock x4 per branch (modules.py:56-72); the branches are independent until the fuse, so the
        // k-th conv1 (then conv2) of every branch goes out as one grouped launch
        for (int k = 0; k < 4; ++k) {
            std::vector<int> t1(nb), g1, g2;
            for (int b = 0; b < nb; ++b) {
                snprintf(buf, sizeof buf, "%s.branches.%d.%d", name.c_str(), b, k);
                const std::string p = buf;
                t1[b] = add_conv(p + ".conv1", p + ".bn1", xs[b], c << b, 3, 1, 1, -1, false);
                g1.push_back((int)convs.size() - 1);
            }
            emit_convs(g1);
            for (int b = 0; b < nb; ++b) {
                snprintf(buf, sizeof buf, "%s.branches.%d.%d", name.c_str(), b, k);
                const std::string p = buf;
                const int t2 = add_conv(p + ".conv2", p + ".bn2", t1[b], c << b, 3, 1, 1, xs[b], false);
                const int i2 = (int)convs.size() - 1, i1 = g1[b];
                // a 48 -> 48 -> 48 block in bf16: both convolutions in one pass over the tile, Y stays in LDS
                const ConvOp &a1 = convs[i1], &a2 = convs[i2];
                if (!disable_bbf && is16() && a1.algo == 1 && a2.algo == 1 && a1.ks == 48 && a1.nr == 3 && a1.slices == 1 &&
                    a1.ntiles == 1 && a2.slices == 1 && a2.ntiles == 1 && conv3x3_lds_bbf_ok(tensors[t2].wp)) {
                    convs[i1].fuse_with = i2;
                    convs[i2].fused_away = true;
                }
                g2.push_back(i2);
                release(t1[b]);
                release(xs[b]);
                xs[b] = t2;
            }
            emit_convs(g2);
        }
        // fuse layers (hrnet.py:25-51, 60-69).  The convolutions feeding the sums are issued level by level -- level 0 =
        // every 1x1 conv and the first conv of every stride-2 chain, level k = the k-th conv of the chains -- so that
        // each level is a handful of grouped launches in which siblings reading the same branch share L2.
        std::vector<std::vector<int>> term(nout, std::vector<int>(nb, -1));
        std::vector<std::vector<int>> cur(nout, std::vector<int>(nb, -1));
        for (int level = 0; level < nb; ++level) {
            std::vector<int> made, dead;
            for (int j = 0; j < nb; ++j) {
                std::vector<int> c1, c2;  // couts of the level's 1x1 / stride-2 readers of branch j
                if (level == 0)
                    for (int i = 0; i < nout && i < j; ++i) c1.push_back(c << i);
                for (int i = j + 1 + level; i < nout; ++i)
                    if (level == 0) c2.push_back(i - j == 1 ? (c << i) : (c << j));
                const int nr1 = (dgroup_nr_mode == 1 && c1.size() > 1) ? common_nr(c1, 1) : 0;
                const int nr2 = (dgroup_nr_mode == 1 && c2.size() > 1) ? common_nr(c2, 2) : 0;
                for (int i = 0; i < nout; ++i) {
                    snprintf(buf, sizeof buf, "%s.fuse_layers.%d.%d", name.c_str(), i, j);
                    const std::string q = buf;
                    if (i < j && level == 0) {  // 1x1 conv + BN, upsample folded into the fuse read (hrnet.py:30-35)
                        term[i][j] = add_conv(q + ".0", q + ".1", xs[j], c << i, 1, 1, 0, -1, false, nr1);
                        made.push_back((int)convs.size() - 1);
                    } else if (i > j && level < i - j) {  // chain of 3x3 s2 convs (hrnet.py:36-51)
                        const bool last = (level == i - j - 1);
                        snprintf(buf, sizeof buf, "%s.%d", q.c_str(), level);
                        const std::string qq = buf;
                        const int src = level == 0 ? xs[j] : cur[i][j];
                        const int nt = add_conv(qq + ".0", qq + ".1", src, last ? (c << i) : (c << j), 3, 2, last ? 0 : 1, -1,
                                                false, level == 0 ? nr2 : 0);
                        made.push_back((int)convs.size() - 1);
                        if (level > 0) dead.push_back(src);
                        cur[i][j] = nt;
                        if (last) term[i][j] = nt;
                    }
                }
            }
            if (made.empty()) break;
            emit_convs(made);
            for (int t : dead) release(t);  // only now: members of one launch must not recycle each other's inputs
        }
        std::vector<int> outs;
        for (int i = 0; i < nout; ++i) {
            std::vector<int> terms, shifts;
            for (int j = 0; j < nb; ++j) {
                terms.push_back(i == j ? xs[j] : term[i][j]);
                shifts.push_back(i < j ? j - i : 0);
            }
            snprintf(buf, sizeof buf, "%s.fuse.%d", name.c_str(), i);
            outs.push_back(add_fuse(terms, shifts, buf));
        }
        {   // the module's outputs are independent: one launch for all of them (HRN_DISABLE_FGROUP: one each)
            const int first = (int)fuses.size() - nout;
            for (int i = 0; i < nout; ++i) {
                fuses[first + i].group = disable_fgroup ? 1 : (i == 0 ? nout : 0);
                if (fuses[first + i].group) ops.push_back({OP_FUSE, first + i});
            }
        }
        for (int i = 0; i < nout; ++i)
            for (int j = 0; j < nb; ++j)
                if (i != j) release(term[i][j]);
        for (int b = 0; b < nb; ++b) release(xs[b]);
        xs = outs;
    }

    // `nblocks` Bottlenecks of 64 planes on a 64-channel input at stride 1 ("layer1" of HRNet and of PoseResNet,
    // modules.py:20-40): in bf16 conv3 of block b and conv1 of block b+1 share the chain kernel
    int add_layer1(int x, int nblocks) {
        char buf[96];
        int o1_next = -1;  // conv1 output of the next Bottleneck when the previous one already produced it
        for (int b = 0; b < nblocks; ++b) {
            snprintf(buf, sizeof buf, "layer1.%d", b);
            const std::string p = buf;
            int o1 = o1_next, r = x;
            const bool chain = is16() && !disable_chain && b < nblocks - 1;
            int ds_idx = -1;
            if (b == 0 && chain && !disable_chain_ds) {
                // the projection shortcut is computed inside the chain kernel: its 256-channel tensor never exists
                o1 = add_conv(p + ".conv1", p + ".bn1", x, 64, 1, 1, 1);
                r = add_conv(p + ".downsample.0", p + ".downsample.1", x, 256, 1, 1, 0, -1, false, 2);
                ds_idx = (int)convs.size() - 1;
                release(r);  // never written: hand the buffer back at once
            } else if (b == 0) {  // conv1 and the projection shortcut both read x: one launch
                o1 = add_conv(p + ".conv1", p + ".bn1", x, 64, 1, 1, 1, -1, false);
                r = add_conv(p + ".downsample.0", p + ".downsample.1", x, 256, 1, 1, 0, -1, false);
                emit_convs({(int)convs.size() - 2, (int)convs.size() - 1});
            } else if (o1 < 0) {
                o1 = add_conv(p + ".conv1", p + ".bn1", x, 64, 1, 1, 1);
            }
            // round 5: blocks whose shortcut is the block input itself (b >= 1) compute their 3x3 in front of conv3 inside the chain
            // kernel -- in the generic kernel's arithmetic (generic weight image, NR = 2), so conv2's own tensor is never written
            // (that arithmetic is taken for these convolutions under EVERY switch setting -- with the fusion or the chain kernel off they
            // run on conv_direct_kernel -- so that all plan variants stay bit-identical)
            const bool c2_generic = is16() && b >= 1;
            const bool chain3 = c2_generic && !disable_chain && !disable_chain3;
            const int o2 = c2_generic ? add_conv(p + ".conv2", p + ".bn2", o1, 64, 3, 1, 1, -1, !chain3, 2, 0, -1, true)
                                      : add_conv(p + ".conv2", p + ".bn2", o1, 64, 3, 1, 1);
            const int i2 = (int)convs.size() - 1;
            int o3;
            o1_next = -1;
            if (chain3 && !chain) {   // the layer's last block: 3x3 + conv3 + shortcut + ReLU, nothing behind
                o3 = add_conv(p + ".conv3", p + ".bn3", o2, 256, 1, 1, 1, r, false, 2);
                chains.push_back({(int)convs.size() - 1, -1, -1, i2});
                ops.push_back({OP_CHAIN, (int)chains.size() - 1});
            } else if (chain) {
                // conv3 (+shortcut, ReLU) of this block and conv1 (+ReLU) of the next in one pass: the 256-channel
                // tensor is written once and never read back by a 1x1 conv (bottleneck_chain.hip)
                snprintf(buf, sizeof buf, "layer1.%d", b + 1);
                const std::string pn = buf;
                o3 = add_conv(p + ".conv3", p + ".bn3", o2, 256, 1, 1, 1, r, false, 2);
                const int i3 = (int)convs.size() - 1;
                o1_next = add_conv(pn + ".conv1", pn + ".bn1", o3, 64, 1, 1, 1, -1, false, 4);
                chains.push_back({i3, (int)convs.size() - 1, ds_idx, chain3 ? i2 : -1});
                ops.push_back({OP_CHAIN, (int)chains.size() - 1});
            } else {
                o3 = add_conv(p + ".conv3", p + ".bn3", o2, 256, 1, 1, 1, r);
            }
            release(o1), release(o2);
            if (b == 0 && ds_idx < 0) release(r);
            release(x);
            x = o3;
        }
        return x;
    }

    // PoseResNet (models_/poseresnet.py:16-122, Bottleneck sizes): 7x7 stem, max-pool, four ResNet layers on the
    // generic / LDS-staged conv kernels, three ConvTranspose2d + BN + ReLU as four 3x3 phase convolutions each, head
    void build_plan_poseresnet() {
        static const int spec50[4] = {3, 4, 6, 3}, spec101[4] = {3, 4, 23, 3}, spec152[4] = {3, 8, 36, 3};
        const int *layers = c == 50 ? spec50 : c == 101 ? spec101 : spec152;
        stem_out_t = new_tensor(64, H / 2, W / 2);
        ops.push_back({OP_STEM7, 0});
        int x = new_tensor(64, H / 4, W / 4);
        pool_in_t = stem_out_t, pool_out_t = x;
        ops.push_back({OP_MAXPOOL, 0});
        release(stem_out_t);
        char buf[96];
        x = add_layer1(x, layers[0]);
        for (int li = 1; li < 4; ++li) {
            const int planes = 64 << li;
            for (int b = 0; b < layers[li]; ++b) {
                snprintf(buf, sizeof buf, "layer%d.%d", li + 1, b);
                const std::string p = buf;
                const int stride = (b == 0 && li > 0) ? 2 : 1;
                int r = x;
                const int o1 = add_conv(p + ".conv1", p + ".bn1", x, planes, 1, 1, 1, -1, false);
                std::vector<int> first{(int)convs.size() - 1};
                if (b == 0) {  // projection shortcut (poseresnet.py:53-59): reads x like conv1
                    r = add_conv(p + ".downsample.0", p + ".downsample.1", x, planes * 4, 1, stride, 0, -1, false);
                    first.push_back((int)convs.size() - 1);
                }
                emit_convs(first);
                const int o2 = add_conv(p + ".conv2", p + ".bn2", o1, planes, 3, stride, 1);
                const int o3 = add_conv(p + ".conv3", p + ".bn3", o2, planes * 4, 1, 1, 1, r);
                release(o1), release(o2);
                if (b == 0) release(r);
                release(x);
                x = o3;
            }
        }
        for (int i = 0; i < 3; ++i) {  // deconv_layers: ConvTranspose2d(4, s2, p1) + BN + ReLU (poseresnet.py:84-104)
            const Tensor tx = tensors[x];
            const int up_t = new_tensor(256, tx.h * 2, tx.w * 2);
            snprintf(buf, sizeof buf, "deconv_layers.%d", 3 * i);
            const std::string cn = buf;
            snprintf(buf, sizeof buf, "deconv_layers.%d", 3 * i + 1);
            const std::string bn = buf;
            std::vector<int> phases;
            for (int ph = 0; ph < 4; ++ph) {
                add_conv(cn, bn, x, 256, 2, 1, 1, -1, false, 0, 1 + ph, up_t);  // k = 2: the four live taps of the phase
                phases.push_back((int)convs.size() - 1);
            }
            emit_convs(phases);
            release(x);
            x = up_t;
        }
        head_in_t = x;
        head_c = tensors[x].c;
        ops.push_back({OP_HEAD, 0});
        ops.push_back({OP_DECODE, 0});
        layout_blob();
    }

    void build_plan() {
        if (model == 1) return build_plan_poseresnet();
        head_c = c;
        // stem conv1 (dedicated kernel), hrnet.py:158-160
        stem_out_t = new_tensor(64, H / 2, W / 2);
        ops.push_back({OP_STEM, 0});
        int x = add_conv("conv2", "bn2", stem_out_t, 64, 3, 2, 1);  // hrnet.py:161-163
        stem_conv2_op = (int)ops.size() - 1;
        // bf16: conv1 + conv2 as ONE kernel (stem_fused.hip) that keeps conv1's output in LDS.  Planned BESIDE the two launches
        // above, which stay the path of a call that taps "stem" and of HRN_DISABLE_STEM_FUSE=1; tile = one output row of conv2
        if (is16() && !disable_stem_fuse && !disable_stem_mfma && stem_fused_fits(tensors[x].wp, W)) {
            stem_fuse = true;
            convs.back().w2_image = true;
            stemf = S2Group();
            stemf.conv_idx = {(int)convs.size() - 1};
            for (int t = 0; t < 2; ++t) {    // 64 couts = two parts of 32 (s2_frags_per_part(64) = 2), one problem
                if (stemf.probs.empty()) {
                    stemf.probs.push_back(S2Group::Prob());
                    stemf.probs[0].in_t = stem_out_t;
                    stemf.probs[0].rows = 1, stemf.probs[0].tiles_per_image = tensors[x].h;
                }
                stemf.probs[0].parts.push_back({(int)convs.size() - 1, t});
            }
        }
        release(stem_out_t);
        char buf[96];
        x = add_layer1(x, 4);  // layer1: Bottleneck x4, modules.py:20-40
        std::vector<int> xs;
        xs.push_back(add_conv("transition1.0.0", "transition1.0.1", x, c, 3, 1, 1, -1, false));
        xs.push_back(add_conv("transition1.1.0.0", "transition1.1.0.1", x, 2 * c, 3, 2, 1, -1, false));
        emit_convs({(int)convs.size() - 2, (int)convs.size() - 1});
        release(x);
        add_stage("stage2.0", xs, 2);
        xs.push_back(add_conv("transition2.2.0.0", "transition2.2.0.1", xs[1], 4 * c, 3, 2, 1));
        for (int m = 0; m < 4; ++m) {
            snprintf(buf, sizeof buf, "stage3.%d", m);
            add_stage(buf, xs, 3);
        }
        xs.push_back(add_conv("transition3.3.0.0", "transition3.3.0.1", xs[2], 8 * c, 3, 2, 1));
        add_stage("stage4.0", xs, 4);
        add_stage("stage4.1", xs, 4);
        add_stage("stage4.2", xs, 1);
        head_in_t = xs[0];
        ops.push_back({OP_HEAD, 0});
        ops.push_back({OP_DECODE, 0});

        layout_blob();
    }

    // Every tensor a launch of the pass writes to HBM, by name (hrn_forward_tap): "stem" (conv1 + bn1 + ReLU), every
    // convolution under its state_dict prefix (its output after bias / residual / ReLU, as stored), "<stage>.fuse.<i>".
    // A tensor stays intact at least until the op after the one that completed it: buffers are recycled by LATER tensors only.
    void index_taps() {
        taps.clear();
        auto add = [&](const std::string &name, int tensor, int op, int conv) {
            for (TapPoint &t : taps)
                if (t.name == name) {  // the four phases of a transposed convolution write one tensor: the last launch completes it
                    t.op = op;
                    return;
                }
            taps.push_back(TapPoint{name, tensor, op, conv});
        };
        for (size_t oi = 0; oi < ops.size(); ++oi) {
            const Op &op = ops[oi];
            switch (op.kind) {
                case OP_STEM:
                case OP_STEM7: add("stem", stem_out_t, (int)oi, -1); break;
                case OP_MAXPOOL: add("maxpool", pool_out_t, (int)oi, -1); break;
                case OP_CONV: add(convs[op.idx].conv, convs[op.idx].out_t, (int)oi, op.idx); break;
                case OP_CONV3_GROUP:
                    for (int ci : groups[op.idx].conv_idx) add(convs[ci].conv, convs[ci].out_t, (int)oi, ci);
                    break;
                case OP_CONV_GROUP:
                    for (int ci : dgroups[op.idx].conv_idx) add(convs[ci].conv, convs[ci].out_t, (int)oi, ci);
                    break;
                case OP_S2_GROUP:
                    for (int ci : s2groups[op.idx].conv_idx) add(convs[ci].conv, convs[ci].out_t, (int)oi, ci);
                    break;
                case OP_CHAIN:  // (the projection shortcut folded into the chain kernel is never written)
                    // and neither is the 3x3's output when the kernel computes it in front of conv3)
                    add(convs[chains[op.idx].conv3].conv, convs[chains[op.idx].conv3].out_t, (int)oi, chains[op.idx].conv3);
                    if (chains[op.idx].conv1 >= 0)
                        add(convs[chains[op.idx].conv1].conv, convs[chains[op.idx].conv1].out_t, (int)oi, chains[op.idx].conv1);
                    break;
                case OP_FUSE:
                    for (int k = 0; k < fuses[op.idx].group; ++k) add(fuses[op.idx + k].name, fuses[op.idx + k].out_t, (int)oi, -1);
                    break;
                default: break;
            }
        }
    }

    void layout_blob() {
        // weight blob layout
        int64_t off = 0;
        stem_w_off = off, off = align_up(off + (model == 1 ? 147 : 27) * 64 * 4, 256);  // PoseResNet: 7x7 stem
        stem_b_off = off, off = align_up(off + 64 * 4, 256);
        stem_wp_off = off, off = align_up(off + (model == 1 ? 5 : 1) * 4 * 1024, 256);  // bf16 MFMA image of conv1 (stem_mfma_kernel / stem7_mfma_kernel)
        for (auto &cv : convs) {
            cv.w_off = off;
            cv.w_bytes = cv.algo == 1 ? (int64_t)cv.ntiles * cv.slices * cv.nch * cv.nr * 1024
                                      : (int64_t)(cv.cout / 16) * cv.kchunks * 1024;
            off = align_up(off + cv.w_bytes, 256);
            cv.b_off = off;
            off = align_up(off + cv.cout * 4, 256);
            if (cv.s2 || cv.w2_image) {  // the slab kernel's image: [cout tile][K chunks][frags][64 lanes][16 B], (48, 3): 14 chunks, (96, 2): 27
                const int nf = s2_frags_per_part(cv.cin);
                cv.w2_off = off;
                cv.w2_bytes = (int64_t)(cv.cout / (16 * nf)) * ((9 * cv.cin + 31) / 32) * nf * 1024;
                off = align_up(off + cv.w2_bytes, 256);
            }
        }
        head_w_off = off, off = align_up(off + (int64_t)joints * head_c * 4, 256);
        head_b_off = off, off = align_up(off + joints * 4, 256);
        // bf16 MFMA image (head_mfma_kernel): one two-fragment image per group of 32 joints, group g behind group g - 1
        head_wp_off = off, off = align_up(off + (int64_t)((joints + 31) / 32) * 2 * ((head_c + 31) / 32) * 1024, 256);
        blob_bytes = off;

        const int hw = (H / 4) * (W / 4);
        head_slab_px = 1024;
        head_slabs = (hw + head_slab_px - 1) / head_slab_px;
        // round 6: calls of a few crops scan 256 pixels per block instead (8 crops of 384x288: 56 blocks of 16 dependent iterations
        // per wave took 24 us for next to no work); the candidate buffers are sized for that split
        head_slabs_small = (hw + kHeadSlabPxSmall - 1) / kHeadSlabPxSmall;
    }

