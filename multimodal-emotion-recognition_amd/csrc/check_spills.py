#!/usr/bin/env python3
"""Build-time guard for gemm.hip (run by the Makefile on hipcc's -Rpass-analysis=kernel-resource-usage remarks).

The k-contiguous staging ring issues its global loads from inline asm and waits with hand-counted vmcnt
(Stage16KC::wait_loaded): the compiler does not know those registers are in flight, so it must never SPILL or move them
between issue and wait - a spilled register is reused for addresses and then overwritten by the landing load (a
512-thread, 128-VGPR build with three register sets did exactly that and faulted).  Every kernel of that form
(m2f_gemm16*<A_RC=false, B_RC=false, ...>, mangled `ILb0ELb0E`) must therefore have zero VGPR spills."""
import re
import sys

# --ring <remarks>: the ring-form kernels (gemm_ring.h) wait for their LDS-DMA loads with hand-counted `s_waitcnt vmcnt(N)`
# (ring_wait_vm): scratch loads / stores are vector-memory operations on the same counter, so ANY scratch use (spills) in
# such a kernel makes the counts wrong - the build must not produce one.
ring = len(sys.argv) > 2 and sys.argv[1] == "--ring"
# --dlong <remarks>: the long-dialogue attention kernels (attention_dlong.hip) keep their output accumulators in registers through
# fully unrolled loops with static indices; an unroll that fails turns them into scratch arrays - refuse the build instead.
dlong = len(sys.argv) > 2 and sys.argv[1] == "--dlong"
# --attn <remarks>: the dialogue attention forward kernels (attention.hip, m2f_attn_fwd_kernel: every NT, with and without a band, with
# and without the distance-decay bias, with and without speaker heads) keep a query tile's scores in registers through fully unrolled loops - the same rule; prints the
# register numbers of each (DESIGN.md section 3 records the biased instantiations beside the ones they were copied from)
attn = len(sys.argv) > 2 and sys.argv[1] == "--attn"
# --stream <remarks>: the streaming attention kernels (attention_stream.hip) - the same rule (a wave's row chunks and accumulators)
stream = len(sys.argv) > 2 and sys.argv[1] == "--stream"
# --stream-chunk <remarks>: its chunk form (attention_stream_chunk.hip) - the same rule (the query block's output accumulators)
stream_chunk = len(sys.argv) > 2 and sys.argv[1] == "--stream-chunk"
# --stream-cache <remarks>: the snapshot / restore kernels of the stream caches (stream_cache.hip) - the same rule (a lane's vectors in flight)
stream_cache = len(sys.argv) > 2 and sys.argv[1] == "--stream-cache"
# --attn-weights <remarks>: the attention-map gather (attention_weights.hip) - the same rule (a tile's accumulators and visibility flags)
attn_weights = len(sys.argv) > 2 and sys.argv[1] == "--attn-weights"
# --w2v <remarks>: the wav2vec2 front end (audio_conv.hip) - the same rule for its kernels (the positional convolution's accumulators)
w2v = len(sys.argv) > 2 and sys.argv[1] == "--w2v"
# --mel <remarks>: the audio_mel encoder (mel_resnet.hip) - the same rule for its kernels (the convolution's accumulators, the STFT sums)
mel = len(sys.argv) > 2 and sys.argv[1] == "--mel"
# --gradnorm <remarks>: the gradient-norm kernels (gradnorm.hip) - the same rule (a slice's loads and float64 accumulators stay in registers)
gradnorm = len(sys.argv) > 2 and sys.argv[1] == "--gradnorm"
# --sam <remarks>: the sharpness-aware minimisation kernels (sam.hip): the finalize launch, the shadow-writing and the flat perturbation for
# fp32 and bf16 gradients, the restore - a tile's loads are all issued before the arithmetic and stay in registers: zero scratch, no
# spills; prints the register numbers of each
sam = len(sys.argv) > 2 and sys.argv[1] == "--sam"
# --tstats <remarks>: the model-watch kernels (tensor_stats.hip) - the same rule (a slice's loads, float64 sums and counters stay in registers)
tstats = len(sys.argv) > 2 and sys.argv[1] == "--tstats"
# --metrics <remarks>: the evaluation-score kernels (metrics.hip) - the same rule (a row's logits and class weights stay in registers)
metrics = len(sys.argv) > 2 and sys.argv[1] == "--metrics"
# --adam <remarks>: the grouped optimizer kernels of adam.hip (parameter groups, AdamW): a group's hyper row must stay in scalar
# registers and a tile's p / g / m / v in vector registers - zero scratch, no spills; prints the register numbers of each.  The same
# rule for the single-group kernels and the exchange kernel, whose EMA forms (the average stream) carry more per tile than they used to
adam = len(sys.argv) > 2 and sys.argv[1] == "--adam"
# --criterion <remarks>: the criterion kernels of rowops.hip (m2f_ce_kernel, m2f_ce_distill_kernel, m2f_ce_focal_kernel,
# m2f_ce_rdrop_kernel: one row definition, criterion_row.h; counted by name below) - the same rule
criterion = len(sys.argv) > 2 and sys.argv[1] == "--criterion"
# --crf <remarks>: the linear-chain CRF kernels (crf.hip) - a lane's transition column / row, its gradient column and the sixteen terms of
# a step stay in registers through unrolled loops with static indices: zero scratch, no spills; prints the register numbers of each
crf = len(sys.argv) > 2 and sys.argv[1] == "--crf"
# --supcon <remarks>: the supervised contrastive kernels (supcon.hip) - a tile's MFMA accumulators, the chunk staged one step ahead and a
# row's terms stay in registers through unrolled loops with static indices: zero scratch, no spills; prints the register numbers of each
supcon = len(sys.argv) > 2 and sys.argv[1] == "--supcon"
# --aux <remarks>: the auxiliary label head's kernels (aux_head.hip) - a row's 16-byte pieces, the sixteen logits, the row's terms and the
# sixteen accumulators of a parameter-gradient lane stay in registers through unrolled loops with static indices: zero scratch, no spills
aux = len(sys.argv) > 2 and sys.argv[1] == "--aux"
# --adv <remarks>: the adversarial ascent kernels (adversarial.hip): the register forms for 1, 2 and 4 pieces per lane and the looping
# form, each per row and per batch, the batch norm's partials and the uniform start - a row's pieces of g, delta and x_clean are all
# loaded before the arithmetic and stay in registers: zero scratch, no spills; prints the register numbers of each
adv = len(sys.argv) > 2 and sys.argv[1] == "--adv"
path = sys.argv[2] if (attn or ring or dlong or stream or stream_chunk or stream_cache or attn_weights or w2v or mel or gradnorm or tstats or metrics or adam or crf or supcon or aux or adv or sam or criterion) else sys.argv[1]
rows, cur = [], None
for line in open(path, errors="replace"):
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}
        rows.append(cur)
    elif cur is not None and "remark" in line:
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m:
            cur["vgpr_spill"] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            cur["scratch"] = int(m.group(1))
        m = re.search(r"\b(VGPRs|AGPRs|TotalSGPRs): (\d+)", line)
        if m:
            cur[m.group(1)] = int(m.group(2))
if adam:
    kernels = [r for r in rows if any(t in r["name"] for t in ("m2f_adam_shadow_grouped", "m2f_adam_slices", "m2f_adam_hyper_groups", "m2f_adam_kernel",
                                                                 "m2f_adam_shadow_kernel", "m2f_ema_exchange"))]
    # grouped shadow-writing and slices: 2 gradient types x with / without the average; the hyper-table refresh; flat and single-group
    # shadow-writing: 4 forms each; the exchange
    if len(kernels) < 18:
        sys.exit(f"check_spills: expected the eighteen optimizer kernels in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if criterion:
    # the four criterion kernels, thin bodies over criterion_row.h's helpers (a row's logits, weights, probabilities and - with a teacher
    # or a twin - the second row's stay in registers): the plain one, the distillation one, the focal one with and without a teacher,
    # the R-Drop one
    kernels = []
    for tag, count in (("m2f_ce_kernel", 1), ("m2f_ce_distill_kernel", 1), ("m2f_ce_focal_kernel", 2), ("m2f_ce_rdrop_kernel", 1)):
        found = [r for r in rows if tag in r["name"]]
        if len(found) != count:
            sys.exit(f"check_spills: expected {count} of {tag} in {path}, found {len(found)} - did the remark format change?")
        kernels += found
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if sam:
    kernels = [r for r in rows if "m2f_sam_" in r["name"]]
    if len(kernels) != 6:
        sys.exit(f"check_spills: expected the six m2f_sam_ kernels in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if adv:
    kernels = [r for r in rows if "m2f_adv_" in r["name"]]
    if len(kernels) != 10:
        sys.exit(f"check_spills: expected the ten m2f_adv_ kernels in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if crf:
    kernels = [r for r in rows if "m2f_crf_" in r["name"]]
    if len(kernels) != 6:
        sys.exit(f"check_spills: expected the six m2f_crf_ kernels in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if supcon:
    kernels = [r for r in rows if "m2f_supcon_" in r["name"]]
    # prep, fwd, rows, bwd, dfeat, the tail with and without accumulation, add
    if len(kernels) != 8:
        sys.exit(f"check_spills: expected the eight m2f_supcon_ kernels in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('AGPRs')} AGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if aux:
    kernels = [r for r in rows if "m2f_aux_" in r["name"]]
    # rows and join for 1, 2 and 4 pieces per lane, the tail with and without accumulation, the gradient's partials and their reduce
    if len(kernels) != 10:
        sys.exit(f"check_spills: expected the ten m2f_aux_ kernels in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('TotalSGPRs')} SGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if attn:
    kernels = [r for r in rows if "m2f_attn_fwd_kernel" in r["name"]]
    if len(kernels) != 32:
        sys.exit(f"check_spills: expected the thirty-two m2f_attn_fwd_kernel instantiations in {path}, found {len(kernels)} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in kernels:
        print(f"check_spills: {r['name']}: {r.get('VGPRs')} VGPRs, {r.get('AGPRs')} AGPRs, {r.get('scratch', 0)} bytes of scratch, "
              f"{r.get('vgpr_spill', 0)} VGPRs spilled", file=sys.stderr if r in bad else sys.stdout)
    sys.exit(1 if bad else 0)
if dlong or stream or stream_chunk or stream_cache or attn_weights or w2v or mel or gradnorm or tstats or metrics:
    tag = "m2f_attn_dlong" if dlong else "m2f_attn_stream" if stream else "m2f_attn_stream_chunk" if stream_chunk else "m2f_stream_cache_kernel" if stream_cache else "m2f_attn_weight" if attn_weights else "m2f_w2v_" if w2v else "m2f_mel_" if mel else "m2f_gradnorm_" if gradnorm else "m2f_tstats_" if tstats else "m2f_eval_"
    kernels = [r for r in rows if tag in r["name"]]
    if not kernels:
        sys.exit(f"check_spills: no {tag} kernel found in {path} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0]
    for r in bad:
        print(f"check_spills: {r['name']} uses {r['scratch']} bytes of scratch per lane", file=sys.stderr)
    sys.exit(1 if bad else 0)
if ring:
    kernels = [r for r in rows if "m2f_gemm16_ring_kernel" in r["name"] or "m2f_gemm_p8_kernel" in r["name"]]
    if not kernels:
        sys.exit(f"check_spills: no ring kernel found in {path} - did the remark format change?")
    bad = [r for r in kernels if r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0]
    for r in bad:
        print(f"check_spills: {r['name']} uses {r.get('scratch', 0)} bytes of scratch per lane ({r.get('vgpr_spill', 0)} VGPRs spilled) "
              "but counts its LDS-DMA loads by hand", file=sys.stderr)
    sys.exit(1 if bad else 0)
bad = [r for r in rows if "m2f_gemm16" in r["name"] and "ILb0ELb0E" in r["name"] and r.get("vgpr_spill", 0) > 0]
checked = sum(1 for r in rows if "m2f_gemm16" in r["name"] and "ILb0ELb0E" in r["name"])
if checked == 0:
    sys.exit("check_spills: no m2f_gemm16 NT kernel found in the remarks - did the remark format change?")
for r in bad:
    print(f"check_spills: {r['name']} spills {r['vgpr_spill']} VGPRs but stages with inline-asm loads", file=sys.stderr)
sys.exit(1 if bad else 0)
