// The DVSR_* environment switches of the native library (A/B aids and kill-switches): one row per switch, one accessor.
// This table is the only statement of a switch's name, scope, parser and default; Python and INTEGRATION.md take theirs from
// it through dvsr_switch_info (include/dynavsr_hip.h), and switches.hip holds the only read of a DVSR_* variable in csrc/.
#pragma once
#include <atomic>

namespace dvsr {

// X(name, scope, parser, default when unset, doc): the variable is DVSR_<name>.
// Scopes (DVSR_SW_<scope>): BUILD read every time a plan is built or an op-level entry chooses a geometry; PROCESS read at the
// switch's own first use and kept; CALL read on every call; DEBUG as CALL, and consumed under -DDVSR_CONV_TRACE only.
// Parsers, of the variable's text once it is set:
//   OFF0 on unless it starts with '0'   ON1 on iff it starts with '1'   INT atoi   SET on, whatever the text (so =0 turns it on)
//   UP2 1 iff it starts with '4'   DCN_FWD 3 empty or s..., 2 r..., else 0   DCN_BWD 1 u..., 2 f..., else 0
#define DVSR_SWITCHES(X) \
  X(CONV_WINO, BUILD, INT, 1, "3x3 stride-1 convs: 0 no Winograd kernel, 1 where the cost model says it is faster, 2 F(2x2) wherever it is eligible") \
  X(CONV_WINO3, BUILD, INT, 1, "0: Winograd F(2x2) on the fp32 pipe and no F(4x4); else on the bf16 pipe with the exact 3-way operand split") \
  X(CONV_WINO5, BUILD, INT, 1, "Winograd F(4x4): 0 never, 1 where the model says it is faster, 2 wherever it is eligible, 3 eligible and 16x32-pixel workgroup tiles") \
  X(CONV_V1, BUILD, ON1, 0, "1: the un-pipelined conv kernel everywhere (no fused activation backward, no per-sample weight sets)") \
  X(EST_SPLIT, BUILD, INT, 1, "0: the estimators' 3x3 convs over padded inputs on the fp32 MFMA kernel instead of the exact 3-way bf16 split") \
  X(EST_SPLIT2, BUILD, INT, 1, "the estimators' 2x2 space-to-depth convs on the bf16 split: 0 none (fp32 MFMA), 1 all, 2 forward launches only") \
  X(FUSE_ACT_BWD, BUILD, OFF0, 1, "0: every activation backward a separate launch") \
  X(BWD_STREAMS, BUILD, OFF0, 1, "0: weight gradients on the launch stream, no side stream") \
  X(PCD_HOIST, BUILD, OFF0, 1, "0: the PCD offset convs convolve the reference frame's half with every frame, not once per clip") \
  X(CONV_LAST_MFMA, PROCESS, ON1, 0, "1: the small-cout 3x3 (conv_last) on the matrix pipe (measured no faster than the VALU kernel)") \
  X(SPLIT_TH8_FROM, PROCESS, INT, 200, "bf16_mfma = 2: 8-row tiles of the split conv kernel from this many workgroups on") \
  X(WGRAD_SPLIT3, PROCESS, OFF0, 1, "0: the plans' 3x3 / 2x2 stride-1 weight gradients stay on the fp32 MFMA kernel") \
  X(WGRAD_WIDE, PROCESS, OFF0, 1, "0: scalar loads in the fp32 and the split weight-gradient kernels") \
  X(WGRAD_S3V, PROCESS, OFF0, 1, "0: the split weight gradient stays on its scalar-staging kernel") \
  X(WGRAD_S3W, PROCESS, OFF0, 1, "0: no eight-wave form of the split weight gradient") \
  X(WGRAD_S3_KYS_BELOW, PROCESS, INT, 4000, "the split weight gradient splits kernel rows below this many tiles x cout blocks x cin blocks (0: never)") \
  X(WGRAD_S3_WGS, PROCESS, INT, 0, "workgroups per row-split launch of the split weight gradient (<= 0: the rule's own 256 / 512)") \
  X(DCN_FWD, PROCESS, DCN_FWD, 3, "deformable-conv forward kernel: split (default), reg (register-staged), dma (any other text)") \
  X(DCN_BWD, PROCESS, DCN_BWD, 0, "deformable-conv backward: unfused = the three-kernel path, fp32 = fp32-MFMA contractions in the fused kernel") \
  X(EST_FUSE_PAD, PROCESS, OFF0, 1, "0: the estimators' reflection pads stay separate launches (default: fused into the producing conv's store)") \
  X(FUSE_RES_BWD, PROCESS, OFF0, 1, "0: skip-connection gradient copies stay separate launches") \
  X(BWD_FORK_EVERY, PROCESS, INT, 0, "layers whose weight gradients share one side-stream fork (1: a fork per layer; <= 0: the plan's own value)") \
  X(BWD_PROBE, PROCESS, OFF0, 1, "0: the shared side stream, unprobed, instead of one measured to run beside the launch stream") \
  X(TSA_DUAL, PROCESS, OFF0, 1, "0: fea_fusion and sAtt_1 as two 1x1 launches instead of one pass over the tensor they share") \
  X(TSA_V, PROCESS, INT, 2, "pixels per thread of the TSA gate kernel: 1, 2 or 4") \
  X(UP2, PROCESS, UP2, 0, "4: the 2x bilinear upsample with four input columns per thread (default: two)") \
  X(DEGRADE_GENERIC, CALL, SET, 0, "set to anything, 0 included: the generic degradation kernel instead of the tiled ones") \
  X(CONV_LDS, DEBUG, INT, 0, "trace build, read per launch: LDS bytes the DMA conv kernel asks for at least (fewer workgroups per CU)") \
  X(CONV_ABLATE, DEBUG, INT, 0, "trace build, kept from its first read, results are WRONG: bit 0 no stores, 1 no halo DMA, 2 no weight DMA, 3 no chunk barriers") \
  X(WGRAD_NOFLUSH, DEBUG, INT, 0, "trace build, kept from its first read, results are WRONG: bit 0 no atomic flush, 1 no loads, 2 no LDS writes, 3 no barriers")

enum class Sw : int {
#define X(name, scope, parser, dflt, doc) name,
  DVSR_SWITCHES(X)
#undef X
  COUNT
};

// sw(Sw::<name>): the switch's parsed value under its scope.  A PROCESS switch, after its first read, costs what the
// function-local static it replaces did: one acquire load, no getenv, no lock.
struct SwKept { std::atomic<bool> known{false}; int value = 0; };
extern SwKept sw_kept[(int)Sw::COUNT];
int sw_read(Sw s);   // getenv + the row's parser; keeps a PROCESS switch's first answer
inline int sw(Sw s) {
  const SwKept& k = sw_kept[(int)s];
  return k.known.load(std::memory_order_acquire) ? k.value : sw_read(s);
}

}  // namespace dvsr
