"""Register / scratch budget of the hot kernels, from the compiler's own metadata (hipcc -S, no GPU needed).
The stage-0 gather runs at 127 of the 128 VGPRs its 16-waves-per-CU launch allows: one more live value and
the compiler spills, which costs 20-150 us per launch (seen with the stamp instrumentation, 56 -> 78 us, and
with an extra kernel argument, 56 -> 202 us).  tests/test_host_api.py runs this as a regression guard."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codenet_amd", "csrc")
# codenet_fused.hip and codenet_pointwise.hip: kernel name fragment -> (max VGPRs incl. AGPRs, or None) ; spills / scratch
# must be zero for all of them
BUDGET = {
    "dw2_kernelILi64ELb0ELb0ELb1ELi1024": 128,    # stage 0, W4A8 (NCHW input, s quantised)
    "dw2_kernelILi64ELb0ELb0ELb0ELi1024": 128,    # stage 0, fp32
    "dw2u_kernelILi64ELb1ELb1": 256,              # stage 1
    "dw2u_kernelILi32ELb1ELb1": 256,              # stage 2
    "pwi8_kernelILi64ELi128ELi2ELb1": 128,        # stages 0-1: four workgroups per CU
    "pwi8_kernelILi128ELi64ELi4ELb1": 128,        # stage 2 (small M)
    "pwi8s_kernelILi4ELi2": 128,                  # stage 0 (round 7): four workgroups per CU, all 1024 resident
    "pwi8s_kernelILi2ELi2": 128,                  # the same for Co <= 64
    "pwi8_kernelILi64ELi64ELi2ELb1": 128,         # Co <= 64 at large M: stage 2, layer 1, heads
    "scale_nchw_kernel": 128, "scale_nhwc_kernelILb1": 128, "unpack_kernelILb1": 128,
    "pwd3_kernelILi2": 256, "pwd3_kernelILi4": 256,   # streaming pointwise: two waves per SIMD
    # 8-bit weight codes (W8A8): a second accumulator set for the high nibble plane -- the 128-column tiles at three
    # workgroups per CU (160 / 148 VGPRs when written), the others at four (88 / 96 / 96)
    "pwi8w_kernelILi64ELi128ELi2ELb1": 168, "pwi8w_kernelILi128ELi64ELi4ELb1": 168,
    "pwi8w_kernelILi32ELi128ELi1ELb1": 128, "pwi8w_kernelILi64ELi64ELi2ELb1": 128,
    "pwi8h_kernelILi2ELi8": 128, "pwi8h_kernelILi3ELi8": 128, "pwi8h_kernelILi4ELi8": 128,
}
# SGPR spills go to VGPR lanes (v_writelane / v_readlane, no memory): tolerated up to this many where listed
SGPR_SPILLS_OK = {"pwd3_kernelILi4": 6}     # round 4: the window cursors of the unit-entry conv (228 VGPRs); round 5: + the NaN flag's mask
# codenet_layers.hip: no spills; the row-streaming kernels must leave two workgroups per CU
BUDGET_LAYERS = {
    "dwx_kernelILb1ELi1ELi2": 256, "dwx_kernelILb1ELi2ELi2": 256,
    "dws_kernelILb1ELi1ELi32ELi1": 256, "dws_kernelILb1ELi1ELi64ELi1": 256, "dws_kernelILb1ELi2ELi32ELi1": 256,
    "head_small_kernelILi0": 256, "head_small_kernelILi1ELi2": 256, "head_small_kernelILi2": 256,
}


# codenet_stage.hip is built WITHOUT the SLP vectoriser (csrc/Makefile): with it the QAT forward
# gather needs 152 VGPRs (three waves per SIMD) instead of 99-106; dcn_generic.hip: the seam's parameter-gradient kernel
# holds a 45-value record per lane under the 128-VGPR cap of its 1024-thread workgroups
BUDGET_STAGE = {"dw4_kernelILb1E": 128, "dw4_kernelILb0E": 128}
BUDGET_GENERIC = {"dwo_wgrad_kernelILi16E": 128, "dwo_wgrad_kernelILi8E": 128,
                  # round 6: the structured forward (four waves per SIMD: 170 VGPRs with a run-time test of the plane
                  # pointer instead of the template parameter) and the structured backward_input kernels (1024-thread
                  # workgroups: 128)
                  "dwo4_kernelILb1E": 128, "dwo4_kernelILb0E": 128,
                  # (the instantiations the CoDeNet stage shapes use: one pass with chunks of 16 / 8, the split form's
                  # grad_input pass with 4 and grad_offset pass with 8; the thin-chunk one-pass forms spill a few VGPRs
                  # and are never launched -- dwos_bwd_split)
                  "dwos_bwd_kernelILi16ELi0E": 128, "dwos_bwd_kernelILi8ELi0E": 128, "dwos_bwd_kernelILi4ELi1E": 128,
                  "dwos_bwd_kernelILi8ELi2E": 128}
SGPR_SPILLS_OK_X = 32      # (SGPR spills go to VGPR lanes: tolerated in the kernels of the two tables below)
# codenet_frozen.hip (round 6): the occupancy the serving network's small launches were measured with -- the 64 x 64
# byte-code pointwise at eight waves per SIMD, the fused depthwise + pointwise at two (256 columns) / three
BUDGET_FROZEN = {"pwq8_kernelILi64ELi64E": 64, "dwpwq8_kernelILi1ELi4ELi2ELi128E": 168, "dwpwq8_kernelILi1ELi4ELi1ELi64E": 168,
                 "dwpwq8_kernelILi2ELi2ELi1ELi64E": 168, "dwpwq8_kernelILi2ELi2ELi2ELi128E": 168,
                 "dwpwq8_kernelILi1ELi4ELi2ELi256ELi32E": 256, "dwpwq8_kernelILi2ELi2ELi2ELi256ELi32E": 256}
# codenet_merge.hip: one 1024-thread workgroup per image (four waves per SIMD: 128 VGPRs); its soft-NMS inner loop
# carries double arithmetic and the double exp -- 74 VGPRs when it was written, no scratch
BUDGET_MERGE = {"merge_scales_kernel": 128}
# codenet_loss.hip: streaming kernels in 256-thread workgroups that hide HBM latency with occupancy -- eight waves per
# SIMD (64 VGPRs) for the two heat-map passes and the finish; the target kernel carries the double exp (four waves)
BUDGET_LOSS = {"ctdet_loss_fwd_kernel": 64, "ctdet_loss_bwd_kernel": 64, "ctdet_loss_finish_kernel": 64,
               "ctdet_targets_kernel": 128}
# codenet_preproc.hip: one thread per output pixel, bound by its stores -- eight waves per SIMD (64 VGPRs; 52 when it was
# written, with the double geometry and the recomputed resize taps), no scratch
# (the crop is a __device__ function shared with crop_sum_kernel: 52 / 51 VGPRs); color_aug_kernel is bound by its 12 bytes
# of stores per pixel: 18 VGPRs when it was written
BUDGET_PREPROC = {"pre_process_kernel": 64, "crop_sum_kernel": 64, "color_aug_kernel": 64}
# codenet_heads_train.hip (built without the SLP vectoriser, as codenet_train.hip): bandwidth-bound register-window
# kernels that hide latency with occupancy -- the depthwise forward and the small tail at eight waves per SIMD (64 VGPRs;
# 46-50 / 37-54 when written), the depthwise backward with its two 3 x 6 windows and ten sums at four (128; 73-104), no
# scratch
BUDGET_HEADS_TRAIN = {"head_dw_fwd_kernel": 64, "head_tail_fwd_kernel": 64, "head_dw_bwd_kernelILi": 128,
                      "train_sums_reduce_kernel": 64}      # (the reduction of units and stem too: cdn_train.h)

# codenet_units_train.hip (built without the SLP vectoriser, as codenet_heads_train.hip): the same kind of bandwidth-bound
# register-window kernels -- the depthwise forward (3 x 6 / 3 x 9 window) and the joins at eight waves per SIMD (64 VGPRs;
# 33-52 / 16-22 when written), the depthwise backward with its input and gradient windows and ten sums at four (128;
# 64-96), no scratch
BUDGET_UNITS_TRAIN = {"unit_dw_fwd_kernel": 64, "unit_join_fwd_kernel": 64, "unit_join_bwd_kernel": 64,
                      "unit_dw_bwd_kernelILi": 128}

# codenet_stem_train.hip (built without the SLP vectoriser, as codenet_units_train.hip): the forward (27 inputs, one
# accumulator at a time) and the pool kernels (a 5 x 5 patch) at eight waves per SIMD (64 VGPRs; 57 / 14 / 50 when written);
# the weight gradient holds 4 x 28 sums beside the 27-value patch and runs at three (168; 160), no scratch
BUDGET_STEM_TRAIN = {"stem_train_fwd_kernel": 64, "stem_pool_fwd_kernel": 64, "stem_pool_bwd_kernel": 64,
                     "stem_wgrad_kernel": 168}

# codenet_bn_train.hip (built without the SLP vectoriser, as codenet_stem_train.hip): streaming kernels bound by HBM, a quad
# per thread and iteration, that hide latency with occupancy -- eight waves per SIMD (64 VGPRs), no scratch, no spills
BUDGET_BN_TRAIN = {"bn_stats_kernel": 64, "bn_apply_kernel": 64, "bn_bwd1_kernel": 64, "bn_bwd2_kernel": 64,
                   "bn_stats_finish_kernel": 64, "bn_bwd_finish_kernel": 64, "bn_eval_stats_kernel": 64}

# codenet_heads_fp32_train.hip (built without the SLP vectoriser, as codenet_bn_train.hip, whose kernels it shares through
# cdn_bn.h): the register-window kernels of the QAT heads with BatchNorm + ReLU formed on load -- the depthwise forward and the
# narrow tail at eight waves per SIMD (64 VGPRs), the depthwise backward with its two 3 x 6 windows, the xh rows and eleven
# float64 sums at four (128); the (channel, slab) kernel of the narrow tail's backward and the pitched second pass at eight;
# no scratch
BUDGET_HEADS_FP32_TRAIN = {"head32_dw_fwd_kernel": 64, "head32_tail_fwd_kernel": 64, "head32_dw_bwd_kernelILb": 128,
                           "head32_tail_bwd_kernelILi": 64, "head32_bn_bwd2_kernel": 64, "head32_tail_bwd_finish_kernel": 64,
                           "dw_bwd_finish_kernel": 64, "bn_stats_kernel": 64, "bn_bwd1_kernelILi1": 64,
                           "bn_stats_finish_kernel": 64, "bn_bwd_finish_kernel": 64, "bn_eval_stats_kernel": 64}
# codenet_units_fp32_train.hip (the fp32 units in training), from the compiled code: the depthwise
# forward 37-62 VGPRs (the scalar stride-2 loader is the widest), the apply / join kernels 21-30, the first backward pass
# 22-36, the depthwise backward 62-93 (stride 1 on the raw input is the widest); no scratch, no spills
BUDGET_UNITS_FP32_TRAIN = {"unit32_dw_fwd_kernel": 64, "unit32_apply_kernel": 32, "unit32_bwd1_kernel": 40,
                           "unit32_dw_bwd_kernelILi": 96, "dw_bwd_finish_kernel": 32}
# codenet_stem_fp32_train.hip (the fp32 stem in training), from the compiled code: the pool forward
# with its 3 x 9 window 41-54 VGPRs, the first backward pass without the pool (cdn_bn.h's bn_bwd1_kernel without its store)
# 22-28, with the pool 52 (the per-pixel gather) and 81 (the 5 x 7 patch of the 16-byte path); the weight gradient holds
# codenet_stem_train.hip's 4 x 28 sums beside the 27-value patch (160, three waves per SIMD); no scratch, no spills
BUDGET_STEM_FP32_TRAIN = {"stem32_pool_fwd_kernel": 64, "stem32_pool_bwd_kernel": 96, "bn_bwd1_kernelILi1": 64,
                          "stem32_wgrad_kernel": 168}
# codenet_eval.hip (detection scoring): float64 box arithmetic in small launches that hide latency
# with occupancy -- eight waves per SIMD (64 VGPRs; 23-60 when written).  The VOC accumulate keeps the explicit stack of
# numpy's pairwise summation (48 frames, thread 0 only, once per class) in private memory: 1360 bytes, no register spills
BUDGET_EVAL = {"eval_append_kernel": 64, "eval_keys_kernel": 64, "eval_match_voc_kernel": 64, "eval_match_coco_kernel": 64,
               "eval_accumulate_voc_kernel": 64, "eval_accumulate_coco_kernel": 64}
SCRATCH_OK = {"eval_accumulate_voc_kernel": 2048}


def kernel_resources(src="codenet_fused.hip", extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "-munsafe-fp-atomics", *extra, "-S", "--cuda-device-only", "-o", out, src],
                       cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
        txt = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size: \d+", txt, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))   # noqa: E731
        res[name] = dict(vgpr=g("vgpr_count"), spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
                         scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"))
    return res


def check():
    res = kernel_resources()
    res.update(kernel_resources("codenet_pointwise.hip"))
    problems = []
    res_l = kernel_resources("codenet_layers.hip")
    for frag, cap in BUDGET_LAYERS.items():
        hits = [(n, r) for n, r in res_l.items() if frag in n]
        if not hits:
            problems.append("kernel %s not found" % frag)
        for n, r in hits:
            # (a few bytes of private segment for a local array are tolerated here: no VGPR spills)
            if r["spill"] or r["sgpr_spill"]:
                problems.append("%s spills: %s" % (n, r))
            if r["vgpr"] > cap:
                problems.append("%s uses %d VGPRs (budget %d)" % (n, r["vgpr"], cap))
    res.update(res_l)
    for src, extra, budget in (("codenet_stage.hip", ("-fno-slp-vectorize",), BUDGET_STAGE), ("dcn_generic.hip", (), BUDGET_GENERIC),
                               ("codenet_frozen.hip", (), BUDGET_FROZEN), ("codenet_merge.hip", (), BUDGET_MERGE),
                               ("codenet_loss.hip", (), BUDGET_LOSS), ("codenet_preproc.hip", (), BUDGET_PREPROC),
                               ("codenet_eval.hip", (), BUDGET_EVAL),
                               ("codenet_heads_train.hip", ("-fno-slp-vectorize",), BUDGET_HEADS_TRAIN),
                               ("codenet_units_train.hip", ("-fno-slp-vectorize",), BUDGET_UNITS_TRAIN),
                               ("codenet_stem_train.hip", ("-fno-slp-vectorize",), BUDGET_STEM_TRAIN),
                               ("codenet_bn_train.hip", ("-fno-slp-vectorize",), BUDGET_BN_TRAIN),
                               ("codenet_heads_fp32_train.hip", ("-fno-slp-vectorize",), BUDGET_HEADS_FP32_TRAIN),
                               ("codenet_units_fp32_train.hip", ("-fno-slp-vectorize",), BUDGET_UNITS_FP32_TRAIN),
                               ("codenet_stem_fp32_train.hip", ("-fno-slp-vectorize",), BUDGET_STEM_FP32_TRAIN)):
        res_x = kernel_resources(src, extra)
        for frag, cap in budget.items():
            hits = [(n, r) for n, r in res_x.items() if frag in n]
            if not hits:
                problems.append("kernel %s not found" % frag)
            sg_ok = 0 if budget is BUDGET_STAGE else SGPR_SPILLS_OK_X
            for n, r in hits:
                if r["spill"] or r["scratch"] > SCRATCH_OK.get(frag, 0) or r["sgpr_spill"] > sg_ok:
                    problems.append("%s spills: %s" % (n, r))
                if r["vgpr"] > cap:
                    problems.append("%s uses %d VGPRs (budget %d)" % (n, r["vgpr"], cap))
        res.update(res_x)
    for frag, cap in BUDGET.items():
        hits = [(n, r) for n, r in res.items() if frag in n]
        if not hits:
            problems.append("kernel %s not found" % frag)
        for n, r in hits:
            if r["spill"] or r["scratch"] or r["sgpr_spill"] > SGPR_SPILLS_OK.get(frag, 0):
                problems.append("%s spills: %s" % (n, r))
            if cap is not None and r["vgpr"] > cap:
                problems.append("%s uses %d VGPRs (budget %d)" % (n, r["vgpr"], cap))
    return res, problems


if __name__ == "__main__":
    res, problems = check()
    for frag in list(BUDGET) + list(BUDGET_STAGE) + list(BUDGET_GENERIC) + list(BUDGET_FROZEN) + list(BUDGET_MERGE) + list(BUDGET_LOSS) + list(BUDGET_PREPROC) + list(BUDGET_EVAL) + list(BUDGET_HEADS_TRAIN) + list(BUDGET_UNITS_TRAIN) + list(BUDGET_STEM_TRAIN) + list(BUDGET_BN_TRAIN) + list(BUDGET_HEADS_FP32_TRAIN) + list(BUDGET_UNITS_FP32_TRAIN) + list(BUDGET_STEM_FP32_TRAIN):
        for n, r in res.items():
            if frag in n:
                print("%-70s %s" % (n[18:88], r))
    if problems:
        print("\n".join(problems))
        sys.exit(1)
    print("ok")
