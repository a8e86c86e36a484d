// struct hrn_ctx, part: the debug switches -- every HRN_* variable a handle reads, each ONCE, when the handle is constructed, in
// this order (hrn_switches() reports what was found in the order of the reads).  Three readers (hrnet_mi355.cpp): sw_set(name) = the
// variable is there; sw_int / sw_real(name, d) = its value, or d without it; sw_zero(name) = it is there and reads as 0.
// Included INSIDE the struct body by hrnet_mi355.cpp (ctx_plan / ctx_memory / ctx_weights / ctx_run / ctx_scratch).
    bool disable_lds = sw_set("HRN_DISABLE_LDS");
    bool assoc_no_assign = sw_set("HRN_ASSOC_NO_ASSIGN");   // timing only: hrn_associate_people_dev skips its assignment phase
    bool disable_group = sw_set("HRN_DISABLE_GROUP");
    bool disable_dgroup = sw_set("HRN_DISABLE_DGROUP");
    bool disable_chain = sw_set("HRN_DISABLE_CHAIN");
    bool small_tiles = !sw_zero("HRN_SMALL_TILES");
    int small_below = sw_int("HRN_SMALL_BELOW", 384);
    int small_keep_above = sw_int("HRN_SMALL_KEEP", 300);   // (0: every convolution of a small launch takes 128-pixel tiles, round 5's rule)
    bool disable_chain_ds = sw_set("HRN_DISABLE_CHAIN_DS");
    // generic conv kernel, bf16: the block's weights through LDS instead of one copy per wave from L2 (+1.6 % on the pass)
    // the K = 64 1x1 convs with a residual fetch it before the K loop (1) or after it (0); persistent blocks of a chain-kernel launch (ADVICE r4: read here, at create,
    // like every other switch -- not in a function-local static at the first launch)
    int pre_mode = sw_int("HRN_PRE_MODE", 1);
    int chain_blocks = sw_int("HRN_CHAIN_BLOCKS", 512);
    // round 5: the 3x3 conv of a Bottleneck without projection shortcut in front of its conv3 inside the chain kernel (off: its own launch)
    bool disable_chain3 = sw_set("HRN_DISABLE_CHAIN3");
    bool direct_wlds = !sw_zero("HRN_DIRECT_WLDS");
    // round 6: stride-2 3x3 convolutions with cin % 32 == 0 on the generic kernel request their pixel fragments two K chunks ahead by
    // LDS-DMA into a per-wave LDS ring (kernels.hip: XL); same arithmetic in the same order: bit-identical to HRN_DIRECT_XLDS=0
    bool direct_xlds = !sw_zero("HRN_DIRECT_XLDS");
    // fused BasicBlocks on the 48-channel branch (conv3x3_lds.hip: bbf_run): bit-identical, 2.5x less HBM traffic on that
    // branch, +2.6 % on the whole pass at 256 crops; HRN_BBF=0 goes back to two launches per block
    bool disable_bbf = sw_zero("HRN_BBF");
    // a fused block walks conv3_tiles_per_block / bbf_tpb_div tiles (short blocks of 1; long ones, 85 % of the tiles, long_factor = 4
    // times that): 64 % of the fused tiles slide (conv1's halo rows carried over, not recomputed).  Longer blocks (2 / 1: 81 / 87 %
    // sliding) measured +0.5 % on two boxes and -4.4 % on a third (profiles/carry_block_length_sweep.txt): not adopted
    int bbf_tpb_div = std::max(1, sw_int("HRN_BBF_TPB_DIV", 3));
    // estimated cost of a sliding tile for the longest-first order, against 28000 for a block's first tile (as the plain blocks'
    // estimates count): the phase stamps measured 21.2 k ticks against 24.1 k
    double bbf_slide_cost = sw_real("HRN_BBF_SLIDE_COST", 24600.0);
    // fused only when the call has at least this many 512-pixel tiles (four per CU): measured at 384x288 +2 % at 256
    // crops (3541 tiles), +1 % at 128-192, +6 % at 96 (1328 tiles), -1 % at 64 (885 tiles), -2 % at 20, -5 % at one crop,
    // where the two plain launches with their smaller tiles spread the work over more CUs
    int bbf_min_tiles = sw_int("HRN_BBF_MIN_TILES", 1100);
    // 1: convolutions that read the same tensor share one cout-tile width so that they can share a launch (and L2)
    int dgroup_nr_mode = sw_int("HRN_DGROUP_NR", 1);
    bool disable_lds32 = sw_set("HRN_DISABLE_LDS32");
    bool disable_n96 = sw_set("HRN_DISABLE_N96");
    bool disable_fgroup = sw_set("HRN_DISABLE_FGROUP");   // one launch per fuse output instead of one per StageModule
    bool disable_f32lds = sw_set("HRN_DISABLE_F32LDS");   // fp32 3x3 stride-1 convs back on the generic kernel
    int f32_small_slices = sw_int("HRN_F32_SMALL_SLICES", 0);   // fp32: 128-pixel tiles from this many slices on (0: never; 4 and 8 measured: no gain)
    // round 4: the 96-cout form enumerates real pixels only (no MFMAs on the pad column / pad row of the flat layout) on grids whose
    // padding is at least this share of the flat pixels; bit-identical to the flat enumeration
    bool disable_compact = sw_set("HRN_DISABLE_COMPACT");
    double compact_min_pad = sw_real("HRN_COMPACT_MIN_PAD", 0.08);
    // stride-2 slab kernel (conv_s2.hip) off: those convolutions stay on the generic kernel (bit-identical results)
    bool disable_s2 = sw_set("HRN_DISABLE_S2");
    // the slab kernel is taken when a launch has at least this many tiles (one per CU); smaller calls use the generic kernel
    int s2_min_tiles = sw_int("HRN_S2_MIN_TILES", 256);
    int s2_target_blocks = std::max(1, sw_int("HRN_S2_BLOCKS", 256));
    bool disable_stem_mfma = sw_set("HRN_DISABLE_STEM_MFMA");
    // round 4: conv1 + conv2 of the stem as one kernel (stem_fused.hip), bit-identical to the two launches it replaces
    bool disable_stem_fuse = sw_set("HRN_DISABLE_STEM_FUSE");
    bool disable_head_mfma = sw_set("HRN_DISABLE_HEAD_MFMA");
    bool direct_nr6 = !sw_zero("HRN_DIRECT_NR6");
    int half_stages_per_block = sw_int("HRN_HALF_STAGES", 8);
    bool alternate = !sw_zero("HRN_ALTERNATE");
    int block_order = sw_int("HRN_BLOCK_ORDER", 1);
    int long_factor = sw_int("HRN_LONG_FACTOR", 4);
    double long_share = sw_real("HRN_LONG_SHARE", 0.85);
