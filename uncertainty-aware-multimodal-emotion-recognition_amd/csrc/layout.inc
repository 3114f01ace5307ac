// The buffers of Stack C's executor, once: X(buffer, kind, name, elements, bf16_only), in the order they lie in their buffer
// (each starts on a 256-byte boundary).  stackc.hip makes struct Layout, make_layout() and the name look-ups
// mmdeer_weights_offset / mmdeer_workspace_offset of this list.
//   buffer     W: the caller's `weights` buffer (mmdeer_weights_bytes) -- ONE set of packed parameters per model, shared by the workspaces
//              of every batch size, written by mmdeer_forward(repack = 1), mmdeer_pack_weights and mmdeer_adamw_step;
//              S: the per-batch workspace (mmdeer_workspace_bytes)
//   kind       ACT: the compute / activation dtype (bf16, or fp32 with compute_f32); BF16; F32
//   elements   in terms of Bz (the batch, at least 1), nblk (nig_nblocks), np / nhead (partial slabs, make_layout()); no parentheses
//   bf16_only  1: empty with compute_f32
X(W, ACT,  wpack,    MMDEER_FLAT_ELEMS, 0)   // the weight matrices at their flat offsets (params.inc)
X(W, ACT,  wtpack,   MMDEER_FLAT_ELEMS, 0)   // transposed weight matrices (W^T) at the same flat offsets: dX runs as an NT GEMM
X(W, F32,  vpack,    MMDEER_FLAT_ELEMS, 0)   // the bias / LayerNorm vectors at their flat offsets
X(W, BF16, wa_pad,   INTER * AUD_PAD, 0)     // bf16 mode: audio_projection.weight as [256][AUD_PAD] (zero-padded rows, 16-byte aligned)
X(W, BF16, wqkv_hm,  3 * FUS * FUS, 0)       // bf16 mode: head-major image of the trimodal in_proj weight for the fused projection + attention kernels
X(W, F32,  wscratch, ADAM_NPART, 0)          // sum-of-squares partials of the optimiser step
X(W, BF16, wfpack,   MMDEER_FLAT_ELEMS, 1)   // fragment-major images (chain.h) of the matrices the forward layer chains stream, at their flat offsets
X(W, BF16, wtfpack,  MMDEER_FLAT_ELEMS, 1)   // the same of the W^T matrices the backward chains stream
X(W, BF16, wa_frag,  INTER * AUD_PAD, 1)     // fragment-major image of wa_pad (the input chain's audio projection)
X(S, BF16, audio_pad, Bz * AUD_PAD, 0)       // bf16 mode: the audio feature block as [B][AUD_PAD]
// saved activations
X(S, ACT, avin, 2 * Bz * INTER, 0) X(S, ACT, avv, 2 * Bz * INTER, 0) X(S, ACT, cat, Bz * 2 * INTER, 0) X(S, ACT, y_a2, Bz * INTER, 0)
X(S, ACT, av, Bz * INTER, 0) X(S, ACT, xtok, 2 * Bz * FUS, 0) X(S, ACT, qkv, 2 * Bz * 3 * FUS, 0) X(S, ACT, obar, Bz * FUS, 0)
X(S, ACT, pool, Bz * FUS, 0) X(S, ACT, y_t3, Bz * FUS, 0) X(S, ACT, tri, Bz * FUS, 0) X(S, ACT, y_o1, Bz * FUS, 0) X(S, ACT, fused, Bz * FUS, 0)
X(S, ACT, h1, Bz * HID, 0) X(S, ACT, h2, Bz * HID, 0) X(S, ACT, e1, Bz * 3 * EV1, 0) X(S, ACT, e2, Bz * 3 * EV2, 0)
X(S, F32, probs, Bz * 8 * 4, 0) X(S, F32, evid, Bz * 12, 0)
X(S, F32, stats, 4 * nblk * 3 * NIG_NSTAT, 0)   // block partials of nig_fwd_kernel, or four wave partials per block (the chain's NIG tail)
X(S, F32, mean_a2, Bz, 0) X(S, F32, rstd_a2, Bz, 0) X(S, F32, mean_t3, Bz, 0) X(S, F32, rstd_t3, Bz, 0) X(S, F32, mean_o1, Bz, 0) X(S, F32, rstd_o1, Bz, 0)
// backward scratch
X(S, ACT, dz2, Bz * 3 * EV2, 0) X(S, ACT, de1, Bz * 3 * EV1, 0) X(S, ACT, dh2, Bz * HID, 0) X(S, ACT, dh1, Bz * HID, 0)
X(S, ACT, dfused, Bz * FUS, 0) X(S, ACT, dz_o1, Bz * FUS, 0) X(S, ACT, dtri, Bz * FUS, 0) X(S, ACT, dz_t3, Bz * FUS, 0)
X(S, ACT, dpool, Bz * FUS, 0) X(S, ACT, dobar, Bz * FUS, 0) X(S, ACT, dqkv, 2 * Bz * 3 * FUS, 0) X(S, ACT, dxtok, 2 * Bz * FUS, 0)
X(S, ACT, dav, Bz * INTER, 0) X(S, ACT, dz_a2, Bz * INTER, 0) X(S, ACT, dcats, 2 * Bz * INTER, 0) X(S, ACT, davv, 2 * Bz * INTER, 0)
X(S, ACT, davin, 2 * Bz * INTER, 0)
// LayerNorm-backward partial slabs: one per workgroup of ln_bwd_kernel, or of the layer chain that ran instead
X(S, F32, part_ln_o1, np * 2 * FUS, 0) X(S, F32, part_ln_t3, np * 2 * FUS, 0) X(S, F32, part_ln_a2, np * 2 * INTER, 0)
// the last head layer's weight / bias gradient partials: one per block of nig_bwd_kernel, or per chain workgroup
X(S, F32, part_w3, nhead * 3 * 256, 0) X(S, F32, part_b3, nhead * 3 * 4, 0)
X(S, F32, slab, SPLITK_MAX * MMDEER_FLAT_ELEMS, 0)   // split-K partial weight gradients: [SPLITK_MAX][MMDEER_FLAT_ELEMS]
