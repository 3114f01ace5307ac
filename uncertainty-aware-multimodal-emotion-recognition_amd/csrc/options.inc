// The launch-plan options, once: X(id, "name", default, lowest, highest).  options.h makes enum OptId of the ids, options.hip the
// table of names, defaults and ranges (mmdeer_set_option refuses a value outside [lowest, highest]: several options index tables).
// The name is the id without OPT_, in lower case: tests/test_cpu_host.py holds every row to that.
X(OPT_FUSED_ATTN, "fused_attn", 1, 0, 1)        // 1: tri_fused.hip (in_proj + attention in one kernel, bf16 mode); 0: the unfused pair (in_proj
                                                // GEMM writing q|k|v + one-wave-per-sample attention kernels) also in bf16 mode
X(OPT_QKV_RECOMPUTE, "qkv_recompute", 1, 0, 1)  // 1: the fused backward recomputes the head tiles; 0 (with the fused forward): the forward also
                                                // stores q|k|v and the backward runs the unfused attention-backward kernel on it
X(OPT_XCD, "xcd", 1, 0, 1)                      // 1: XCD-contiguous workgroup renumbering in the GEMM kernels
X(OPT_NT128, "nt128", 1, 0, 1)                  // 1: one 8-wave 128x128 LDS-DMA workgroup per CU where 128x64 tiles would need two
X(OPT_NT192, "nt192", 1, 0, 1)                  // 1: 256x192 tiles in the 256-row forward kernel when they fill the chip in one round
X(OPT_GLDS, "glds", 1, 0, 1)                    // 1: LDS-DMA GEMM kernels; 0: register-staged kernels everywhere (A/B comparison, debugging)
X(OPT_NT8, "nt8", 1, 0, 1)                      // 1: the 8-wave 128x64 form of the LDS-DMA kernel; 0: never
X(OPT_T128, "t128", 512, 1, 1 << 30)            // smallest 128x64 tile count that selects the 128x64 kernel
X(OPT_TILE, "tile", -1, -1, 4)                  // -1: automatic; 0..4: force a GemmTile
X(OPT_KSTEPS, "ksteps", 0, 0, 4096)             // 0: automatic; > 0: K-tiles per split-K slice of a weight-gradient problem
X(OPT_LN_FUSED, "ln_fused", 1, 0, 1)            // 1: every LayerNorm of the forward runs inside the GEMM that consumes it (gemm_ln.hip, bf16 mode)
X(OPT_CHAIN, "chain", 1, 0, 1)                  // 1: the row-local layer chains of the forward run as single launches (chain.hip, bf16 mode)
X(OPT_CHAIN_BWD, "chain_bwd", 1, 0, 1)          // 1 (with chain = 1): the head / trimodal dX products and LayerNorm backwards of the backward pass as one chain launch
X(OPT_CHAIN_MIN, "chain_min", 512, 1, 1 << 30)  // smallest batch that takes the chains (default 512: measured wins down to there; tests lower it)
X(OPT_DW_TILE, "dw_tile", 2, 2, 4)              // GemmTile of the weight-gradient launch: 2 = 128x128 tiles without split-K (default), 3 = 256x256 + split-K slabs, 4 = 256x128
X(OPT_DW_KG, "dw_kg", 2, 1, 2)                  // 128x128 weight-gradient tiles: 2 = the workgroup's halves split each 64-row stage of K (default), 1 = 32-row stages
X(OPT_CHAIN_MAX, "chain_max", 8192, 1, 1 << 30) // largest batch that takes the chains
X(OPT_CHAIN_NIG, "chain_nig", 1, 0, 1)          // 1 (with the backward chain, loss mode): the head's last-layer backward + loss gradient run in the chain's prologue
X(OPT_SPLITK_MAX, "splitk_max", 8, 1, 8)        // largest number of split-K slices of a weight-gradient problem (slabs: 4 B per parameter per slice)
X(OPT_CHAIN_DEPTH, "chain_depth", 4, 2, 8)      // weight stages a wave of the 16-sample layer-chain kernel keeps in flight: 4 (default), 2, or 8 (two granules of four
                                                // slots: parity-green, measured slower -- register spills at 192 compiler-visible registers)
X(OPT_CHAIN_TS, "chain_ts", 0, 0, 32)           // 0: 16-sample chain workgroups up to B = 4096, 32-sample ones above; 16 / 32: that size at every batch
X(OPT_CHAIN_IN, "chain_in", 1, 0, 1)            // 1 (with chain = 1, bf16 feature blocks, B <= 4096): the three input projections and the audio padding run
                                                // inside the audio-visual chain's launch instead of as pad + F1 launches
X(OPT_CHAIN_NIGF, "chain_nigf", 0, 0, 1)        // 1 (with chain = 1; default 0): the NIG head (last layer, activations, loss statistics) runs as the tail of the
                                                // forward head chain instead of a launch of its own.  Bit-identical, one launch fewer -- and measured 6 us
                                                // SLOWER per step at B = 4096: the 256 wave partials cost the backward chain's prologue 8k cycles more to
                                                // fetch than the 64 block partials, the tail itself 5k (DESIGN.md)
X(OPT_ADAM_FUSED, "adam_fused", 1, 0, 1)        // 1 (bf16 mode): mmdeer_adamw_step writes every derived weight image from the update itself, tile by tile (optim.h);
                                                // 0: element-wise update + one repack launch
X(OPT_DW_FOLD, "dw_fold", 1, 0, 1)              // 1 (bf16 mode, all weight gradients in one launch of the DMA kernel): that launch adds its own K-slices, folds the row
                                                // partials in workgroups behind its tiles and bumps the dropout counter; 0: the reduce_partials launch behind it
