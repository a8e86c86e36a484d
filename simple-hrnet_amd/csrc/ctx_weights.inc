// struct hrn_ctx, part: state_dict ingestion -- by-name lookup, BatchNorm fold, MFMA-fragment packing (SimpleHRNet.py:117-121).
// Included INSIDE the struct body by hrnet_mi355.cpp (member functions defined in place; one type, split by concern:
// ctx_plan / ctx_memory / ctx_weights / ctx_run).
    // ---------------------------------------------------------------- weights
    struct Src {
        const float *p = nullptr;
        int64_t count = 0;
    };

    bool lookup(const std::map<std::string, Src> &m, const std::string &key, int64_t expect, const float **out) {
        auto it = m.find(key);
        if (it == m.end()) {
            err = "state_dict is missing key '" + key + "'";
            return false;
        }
        if (it->second.count != expect) {
            err = "state_dict key '" + key + "' has " + std::to_string(it->second.count) + " elements, expected " +
                  std::to_string(expect);
            return false;
        }
        *out = it->second.p;
        return true;
    }

    // scale/shift of an eval-mode BatchNorm2d (eps 1e-5): y = x*scale + shift
    bool bn_fold(const std::map<std::string, Src> &m, const std::string &bn, int ch, std::vector<double> &scale,
                 std::vector<double> &shift) {
        const float *g, *b, *mu, *var;
        if (!lookup(m, bn + ".weight", ch, &g) || !lookup(m, bn + ".bias", ch, &b) ||
            !lookup(m, bn + ".running_mean", ch, &mu) || !lookup(m, bn + ".running_var", ch, &var))
            return false;
        scale.resize(ch), shift.resize(ch);
        for (int i = 0; i < ch; ++i) {
            scale[i] = (double)g[i] / std::sqrt((double)var[i] + 1e-5);
            shift[i] = (double)b[i] - (double)mu[i] * scale[i];
        }
        return true;
    }

    bool load_weights(const hrn_tensor_desc *descs, int n) {
        std::map<std::string, Src> m;
        for (int i = 0; i < n; ++i) {
            if (descs[i].dtype != HRN_T_F32 || !descs[i].data || !descs[i].name) continue;
            int64_t cnt = 1;
            for (int d = 0; d < descs[i].ndim; ++d) cnt *= descs[i].dims[d];
            m[descs[i].name] = Src{(const float *)descs[i].data, cnt};
        }
        std::vector<char> host((size_t)blob_bytes, 0);
        pack_overflow = false;
        std::vector<double> scale, shift;
        if (model == 1) {  // PoseResNet stem: w[k = (ci*7 + kh)*7 + kw][co]
            const float *w;
            if (!lookup(m, "conv1.weight", 64 * 147, &w) || !bn_fold(m, "bn1", 64, scale, shift)) return false;
            float *dw = (float *)(host.data() + stem_w_off), *db = (float *)(host.data() + stem_b_off);
            for (int co = 0; co < 64; ++co) {
                for (int k = 0; k < 147; ++k) dw[k * 64 + co] = (float)((double)w[co * 147 + k] * scale[co]);
                db[co] = (float)shift[co];
            }
            // MFMA image: five K chunks (k = (ci*7 + kh)*7 + kw, zero for k >= 147), 4 fragments, cout permutation NR = 4
            uint16_t *dp = (uint16_t *)(host.data() + stem_wp_off);
            for (int kc = 0; kc < 5; ++kc)
                for (int j = 0; j < 4; ++j)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int li = lane & 15, g = lane >> 4;
                        const int co = (li >> 2) * 16 + j * 4 + (li & 3);
                        for (int e = 0; e < 8; ++e) {
                            const int k = kc * 32 + g * 8 + e;
                            dp[((kc * 4 + j) * 64 + lane) * 8 + e] =
                                to16(k < 147 ? (float)((double)w[co * 147 + k] * scale[co]) : 0.f);
                        }
                    }
        } else {  // stem: w[k = ci*9+kh*3+kw][co]
            const float *w;
            if (!lookup(m, "conv1.weight", 64 * 27, &w) || !bn_fold(m, "bn1", 64, scale, shift)) return false;
            float *dw = (float *)(host.data() + stem_w_off), *db = (float *)(host.data() + stem_b_off);
            for (int co = 0; co < 64; ++co) {
                for (int k = 0; k < 27; ++k) dw[k * 64 + co] = (float)((double)w[co * 27 + k] * scale[co]);
                db[co] = (float)shift[co];
            }
            // MFMA image: one K chunk (k = ci*9 + kh*3 + kw, zero for k >= 27), 4 fragments, the usual cout
            // permutation with NR = 4 (lane owns 16 contiguous channels)
            uint16_t *dp = (uint16_t *)(host.data() + stem_wp_off);
            for (int j = 0; j < 4; ++j)
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, g = lane >> 4;
                    const int co = (li >> 2) * 16 + j * 4 + (li & 3);
                    for (int e = 0; e < 8; ++e) {
                        const int k = g * 8 + e;
                        dp[(j * 64 + lane) * 8 + e] = to16(k < 27 ? (float)((double)w[co * 27 + k] * scale[co]) : 0.f);
                    }
                }
        }
        std::vector<float> wf;
        for (auto &cv : convs) {
            const float *w;
            const int kk = cv.k * cv.k, K = kk * cv.cin;
            if (cv.up) {
                // phase (a, b) of ConvTranspose2d(cin, cout, 4, stride 2, padding 1), weight [ci][co][ky][kx]:
                // out(2y + a, 2x + b) = sum over input (y + dy, x + dx) with ky = a + 1 - 2*dy in [0, 4), i.e.
                // a = 0: (dy 0, ky 1), (dy -1, ky 3);  a = 1: (dy +1, ky 0), (dy 0, ky 2) -- the same along x.
                if (!lookup(m, cv.conv + ".weight", (int64_t)cv.cin * cv.cout * 16, &w) ||
                    !bn_fold(m, cv.bn, cv.cout, scale, shift))
                    return false;
                const int a = (cv.up - 1) >> 1, b = (cv.up - 1) & 1;
                wf.assign((size_t)cv.cout * K, 0.f);   // K = 4*cin: live tap t = ty*2 + tx, dy = ty - 1 + a, dx = tx - 1 + b
                for (int t = 0; t < 4; ++t) {
                    const int dy = (t >> 1) - 1 + a, dx = (t & 1) - 1 + b;
                    const int ky = a + 1 - 2 * dy, kx = b + 1 - 2 * dx;   // in [0, 4) by construction
                    for (int co = 0; co < cv.cout; ++co)
                        for (int ci = 0; ci < cv.cin; ++ci)
                            wf[(size_t)co * K + t * cv.cin + ci] =
                                (float)((double)w[(((size_t)ci * cv.cout + co) * 4 + ky) * 4 + kx] * scale[co]);
                }
                pack_conv(cv, wf.data(), K, host.data() + cv.w_off);
                float *db = (float *)(host.data() + cv.b_off);
                for (int co = 0; co < cv.cout; ++co) db[co] = (float)shift[co];
                continue;
            }
            if (!lookup(m, cv.conv + ".weight", (int64_t)cv.cout * K, &w) ||
                !bn_fold(m, cv.bn, cv.cout, scale, shift))
                return false;
            // fold + reorder OIHW -> [co][tap*cin + ci]
            wf.assign((size_t)cv.cout * K, 0.f);
            for (int co = 0; co < cv.cout; ++co)
                for (int ci = 0; ci < cv.cin; ++ci)
                    for (int t = 0; t < kk; ++t)
                        wf[(size_t)co * K + t * cv.cin + ci] =
                            (float)((double)w[((size_t)co * cv.cin + ci) * kk + t] * scale[co]);
            if (cv.algo == 1)
                pack_conv_lds(cv, wf.data(), K, host.data() + cv.w_off);
            else
                pack_conv(cv, wf.data(), K, host.data() + cv.w_off);
            if (cv.s2 || cv.w2_image) {
                ConvOp img = cv;   // same folded weights as ONE slice of all cin channels: k = tap * cin + ci, as the generic kernel orders it
                img.ks = cv.cin, img.nr = s2_frags_per_part(cv.cin), img.slices = 1, img.ntiles = cv.cout / (16 * img.nr);
                img.nch = (9 * cv.cin + 31) / 32, img.n96 = false;
                pack_conv_lds(img, wf.data(), K, host.data() + cv.w2_off);
            }
            float *db = (float *)(host.data() + cv.b_off);
            for (int co = 0; co < cv.cout; ++co) db[co] = (float)shift[co];
        }
        {
            const float *w, *b;
            const int c = head_c;  // channels final_layer reads
            if (!lookup(m, "final_layer.weight", (int64_t)joints * c, &w) || !lookup(m, "final_layer.bias", joints, &b))
                return false;
            memcpy(host.data() + head_w_off, w, sizeof(float) * joints * c);
            memcpy(host.data() + head_b_off, b, sizeof(float) * joints);
            // MFMA image of joint group gr (joints 32 gr ..): fragment f, chunk kc, lane (li, g): joint 32*gr + f*16 + li,
            // k = kc*32 + g*8 + e; rows past the last joint are zero.  Group gr lies behind group gr - 1, each the image a head of
            // those 32 joints alone would have.
            const int kch = (c + 31) / 32;
            uint16_t *img = (uint16_t *)(host.data() + head_wp_off);
            for (int gr = 0; gr < (joints + 31) / 32; ++gr)
                for (int f = 0; f < 2; ++f)
                    for (int kc = 0; kc < kch; ++kc)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 8; ++e) {
                                const int j = gr * 32 + f * 16 + (lane & 15), k = kc * 32 + (lane >> 4) * 8 + e;
                                img[((size_t)((gr * 2 + f) * kch + kc) * 64 + lane) * 8 + e] =
                                    (j < joints && k < c) ? to16(w[(size_t)j * c + k]) : (uint16_t)0;
                            }
        }
        if (pack_overflow) {
            err = "a folded weight exceeds 65504 in magnitude: it has no fp16 representation (use dtype bf16 or fp32)";
            return false;
        }
        if (plan_only) {
            memcpy(blob, host.data(), (size_t)blob_bytes);
        } else {
            if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return false;
            if (!hip_ok(hipMemcpy(blob, host.data(), (size_t)blob_bytes, hipMemcpyHostToDevice), "hipMemcpy(weights)"))
                return false;
        }
        weights_loaded = true;
        return true;
    }

    // one folded weight in the handle's 16-bit format (bf16 / fp16, round to nearest even); an fp16 magnitude above 65504 is
    // noted and fails the load
    mutable bool pack_overflow = false;
    uint16_t to16(float v) const {
        if (dtype != HRN_F16) return f32_to_bf16_host(v);
        if (std::fabs(v) > 65504.f) pack_overflow = true;
        return f32_to_f16_host(v);
    }

    // Fragment-major packing (DESIGN.md §4).  One fragment = 16 packed rows x one K-chunk = 64 lanes x 16 B,
    // stored lane-linear so a wave loads it with one coalesced 1 KiB access.  Fragment f = ng*NR + j holds,
    // in packed row i (= lane & 15), output channel  ng*16*NR + (i>>2)*4*NR + j*4 + (i&3); lane group
    // g = lane>>4 holds k = kc*KC + g*VEC + [0,VEC).  With the operand swap D = W * X^T each lane then owns
    // 4*NR contiguous channels of one pixel.
    void pack_conv(const ConvOp &cv, const float *wf, int K, char *dst) const {
        const int KC = is16() ? 32 : 16, VEC = is16() ? 8 : 4;
        const int nfrag = cv.cout / 16;
        for (int f = 0; f < nfrag; ++f) {
            const int ng = f / cv.nr, j = f % cv.nr;
            for (int kc = 0; kc < cv.kchunks; ++kc)
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, g = lane >> 4;
                    const int co = ng * 16 * cv.nr + (li >> 2) * 4 * cv.nr + j * 4 + (li & 3);
                    char *d = dst + (((size_t)f * cv.kchunks + kc) * 64 + lane) * 16;
                    for (int e = 0; e < VEC; ++e) {
                        const int k = kc * KC + g * VEC + e;
                        const float v = k < K ? wf[(size_t)co * K + k] : 0.f;
                        if (is16())
                            ((uint16_t *)d)[e] = to16(v);
                        else
                            ((float *)d)[e] = v;
                    }
                }
        }
    }

    // Slice-major image for conv3x3_lds_kernel: block (cout tile t, slice s) is the exact LDS image
    // [chunk c][frag j][lane][8 bf16]; within a slice k = tap*KS + ci_local, zero beyond 9*KS.
    void pack_conv_lds(const ConvOp &cv, const float *wf, int K, char *dst) const {
        const int KS = cv.ks, NRB = cv.nr;
        if (KS == 16) {  // fp32 form (conv3x3_f32.hip): [cout tile][slice][9 taps][frag][lane][4 fp32], k = 4 g + e of the slice's 16
            for (int t = 0; t < cv.ntiles; ++t)
                for (int s = 0; s < cv.slices; ++s) {
                    float *blk = (float *)(dst + ((size_t)t * cv.slices + s) * cv.nch * NRB * 1024);
                    for (int c = 0; c < 9; ++c)
                        for (int j = 0; j < NRB; ++j)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int li = lane & 15, g = lane >> 4;
                                const int co = t * 16 * NRB + (li >> 2) * 4 * NRB + j * 4 + (li & 3);
                                for (int e = 0; e < 4; ++e)
                                    blk[((size_t)(c * NRB + j) * 64 + lane) * 4 + e] = wf[(size_t)co * K + c * cv.cin + s * 16 + 4 * g + e];
                            }
                }
            return;
        }
        for (int t = 0; t < cv.ntiles; ++t)
            for (int s = 0; s < cv.slices; ++s) {
                uint16_t *blk = (uint16_t *)(dst + ((size_t)t * cv.slices + s) * cv.nch * NRB * 1024);
                for (int c = 0; c < cv.nch; ++c)
                    for (int j = 0; j < NRB; ++j)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int li = lane & 15, g = lane >> 4;
                            // (96-cout form: conv3x3_n96.inc N96_CH64 -- a lane's channels are 8 contiguous ones per 32-channel group)
                            const int co = (cv.n96 && conv3x3_n96_ch64()) ? t * 96 + (j >> 1) * 32 + (li >> 2) * 8 + (j & 1) * 4 + (li & 3)
                                                                          : t * 16 * NRB + (li >> 2) * 4 * NRB + j * 4 + (li & 3);
                            uint16_t *d = blk + ((size_t)(c * NRB + j) * 64 + lane) * 8;
                            for (int e = 0; e < 8; ++e) {
                                const int kl = 32 * c + 8 * g + e;
                                float v = 0.f;
                                if (kl < 9 * KS) {
                                    const int tap = kl / KS, cil = kl % KS;
                                    v = wf[(size_t)co * K + tap * cv.cin + s * KS + cil];
                                }
                                d[e] = to16(v);
                            }
                        }
            }
    }

