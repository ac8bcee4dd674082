/*
 * libxsmm_hip.h -- the GPU-side additions to the LIBXSMM dispatch/param API.
 *
 * Nothing in here exists in the reference: the reference executes one tiny kernel per
 * synchronous call on host pointers and leaves batching/threading to the caller's
 * OpenMP loop [ref: documentation/libxsmm_mm.md:95-107].  A GPU needs the caller's
 * loop *inside* one launch, a stream to order work on, and device memory.  These entry
 * points provide exactly that and nothing else; every one of them is plain C ABI
 * (pointers and sizes, no HIP or torch types in the signatures).
 *
 * Semantics of the batched launchers -- the contract the parity tests check:
 *
 *   libxsmm_hip_gemm_batch_strided(f, p, count, sa, sb, sc)
 *     ==  for (i = 0; i < count; ++i) { q = *p;
 *            q.a.primary = (char*)p->a.primary + i*sa;
 *            q.b.primary = (char*)p->b.primary + i*sb;
 *            q.c.primary = (char*)p->c.primary + i*sc;  f(&q); }
 *
 * i.e. the caller's loop over independent (BR)GEMMs, with byte strides applied to the
 * `primary` slots (a stride of 0 shares the operand across the batch, e.g. weights).
 * In BATCH_REDUCE_ADDRESS mode a/b.primary are pointer arrays, so sa/sb step through
 * those arrays (sa = br_count*sizeof(void*) gives each batch element its own list).
 * op.tertiary (br_count), a/b.secondary (offset arrays) are shared by all elements.
 * MXFP4 weights: the E8M0 scales in a.tertiary step with A -- by sa*2/32 bytes (one scale byte per 32 weights; sa must be
 * a multiple of 16), or by sa through the list of per-block scale pointers in BATCH_REDUCE_ADDRESS mode.
 *
 * The same call accepts a packed sparse handle (libxsmm_create_packed_spgemm_csr/_csc, _spgemm_csr_areg, FsSpMDM kernels):
 * the loop over element-local packed tensors an application like EDGE runs around one small operator
 * [ref: samples/edge]. The sparse operand's values are shared, so its stride must be 0 (anything else is an error);
 * the dense operand and C step by sb/sa and sc.  A kernel whose single call was too small to specialise is
 * specialised by the first eager batched launch that covers enough columns.
 */
#ifndef LIBXSMM_HIP_H
#define LIBXSMM_HIP_H

#if !defined(LIBXSMM_H)
# error include libxsmm.h, not libxsmm_hip.h
#endif

/* ---- device, stream and synchronisation policy (state is per host thread) --------- */
/** Number of visible HIP devices (0 if none: every dispatch then returns NULL). */
LIBXSMM_API int libxsmm_hip_device_count(void);
/** Select the device used by the calling thread for subsequent dispatch/launches. */
LIBXSMM_API int libxsmm_hip_set_device(int device);
LIBXSMM_API int libxsmm_hip_get_device(void);
/**
 * Launch on the given hipStream_t (passed as void*; NULL = the legacy default stream) and
 * switch the calling thread to stream-ordered (asynchronous) execution: a kernel call
 * returns after enqueueing, results are valid in stream order.
 */
LIBXSMM_API void libxsmm_hip_set_stream(void* hip_stream);
LIBXSMM_API void* libxsmm_hip_get_stream(void);
/**
 * 0 (default, also LIBXSMM_HIP_SYNC=1): every kernel call blocks until C is valid, which
 * is the reference's semantics.  1: stream-ordered.  LIBXSMM_HIP_ASYNC=1 presets it.
 * 2 (LIBXSMM_HIP_ASYNC=2 or LIBXSMM_HIP_COALESCE=1): stream-ordered AND coalescing -- the reference leaves the batch loop to the caller
 * (one small GEMM per call [ref: documentation/libxsmm_mm.md:95-107]); in this mode consecutive calls through ONE plain GEMM / stride-BRGEMM handle
 * are queued (three pointers per call, nothing is launched) and leave as ONE pointer-list batch launch when anything else happens: a call through
 * another handle or kind, another batch-reduce count, libxsmm_hip_sync / _set_stream / _set_async / libxsmm_finalize / libxsmm_release_kernel, 65 536
 * queued calls, or a call that reads or writes what a queued call writes (or writes what one reads): the caller's dependent sequences keep their
 * order.  An unmodified `for (i...) kernel(&param_i);` loop followed by libxsmm_hip_sync() thus runs as one batched launch.  Operands must be
 * device-accessible (as in mode 1); calls with a fused operator, pointer / offset lists or per-call scale operands are not queued (they launch as in mode 1).
 */
LIBXSMM_API void libxsmm_hip_set_async(int enable);
LIBXSMM_API int libxsmm_hip_get_async(void);
/**
 * What the calling thread's next launches should assume about their dense operands -- the read-side counterpart of the reference's
 * non-temporal-store hint for C [ref: include/libxsmm_typedefs.h LIBXSMM_GEMM_FLAG_ALIGN_C_NTS_HINT]:
 *   0 (default, also LIBXSMM_HIP_STREAMING=0): decide per launch -- operands of a launch that moves more than the 256 MiB Infinity Cache
 *     holds are loaded non-temporally (they cannot be resident); so are the operands of a smaller launch when the thread's recent launches on OTHER
 *     operand sets (the last 32 sets, each forgotten after 96 launches) together with this one exceed the cache -- a caller that walks over more
 *     input than the cache holds re-reads nothing from it either (round 6); a caller that keeps launching on the same resident set stays cacheable,
 *     and so does a launch whose first operand is what one of those recent launches wrote (a hand-over inside a chain: GEMM, then a TPP on its C);
 *   1: operands are re-read by later launches or were just produced on the device (keep them cacheable, never non-temporal);
 *   2: operands are read once from HBM (a pass over a working set far larger than the cache): non-temporal loads at every size.
 * Measured on 4096 f32 32^3 problems: hint 2 is 7 % faster when the operands do come from HBM and 50 % slower when they were
 * resident in the Infinity Cache, which is why it is not a default; since round 6 mode 0 makes the same choice as the right
 * declaration in both cases (one resident set 5.69 / 5.68 / 9.06 us for modes 0 / 1 / 2, twelve rotated sets 9.97 / 10.74 / 9.99 us).
 * libxsmm_hip_streaming_window_verdict(): what mode 0's look at the recent launches said for the calling thread's last launch (1: they exceed the cache).
 */
LIBXSMM_API void libxsmm_hip_set_streaming_hint(int mode);
LIBXSMM_API int libxsmm_hip_get_streaming_hint(void);
LIBXSMM_API int libxsmm_hip_streaming_window_verdict(void);
/** Block until all work enqueued by the calling thread's stream has finished. */
LIBXSMM_API void libxsmm_hip_sync(void);
/** Pipeline section: the calling thread DECLARES that the kernel launches it issues between _begin and _end are mutually independent (no launch reads
 * what another one of the section writes) and may overlap on the device.  A launch of a few thousand small problems is one round of waves: a third of
 * its time is filling and draining the chip (the headline launch sits on the copy floor of its footprint), and back-to-back launches on one
 * stream cannot overlap that.  Inside a section consecutive launches rotate over `lanes` (2..8) internal streams: _begin forks them off the thread's stream
 * (they wait for everything issued to it before), _end joins them back (the thread's stream waits for every lane); everything is stream-ordered, so a
 * section may be captured into a hipGraph (the lanes become parallel branches).  Needs stream-ordered launches (libxsmm_hip_set_stream / _set_async);
 * libxsmm_hip_sync and libxsmm_hip_set_stream close an open section.  Each lane has its own partial-result workspace. */
LIBXSMM_API int libxsmm_hip_pipeline_begin(int lanes);
LIBXSMM_API int libxsmm_hip_pipeline_end(void);
/** Capture-time fusion.  While a stream is being captured into a hipGraph, consecutive strided-batch launches of the lean f32 kernel (32 x 32 problems, 16-byte
 * aligned C, non-negative 32-bit batch strides) through ONE handle with the same count, strides and batch-reduce count are folded into one kernel node when
 * the new launch is address-independent of every launch already in the node: its C range meets none of their A, B or C ranges and their C ranges meet neither
 * its A nor its B range (bounding intervals base ... base + (count - 1) * stride + extent; ranges that only touch are independent).  The graph stays a linear
 * chain with fewer, larger kernel nodes; results are bit for bit those of the separate launches.  What the caller can see: an event recorded between two fused
 * launches completes after both.  Anything else on the stream between two launches (another kernel, a copy, a wait on another stream) ends the run, as does a
 * pipeline section.  Nothing changes outside a capture.
 * max_launches: the most launches one node may hold; 0 or 1 = off; values above the built-in limit (16) are lowered to it.  Returns the previous value.
 * Process-wide, on by default; LIBXSMM_HIP_CAPTURE_FUSION=0 starts with it off (any other number presets max_launches).  If a graph call fails the launch is
 * issued on its own, fusion switches itself off for the process and the thread's error state says why. */
LIBXSMM_API int libxsmm_hip_set_capture_fusion(int max_launches);
/** Number of calls of the calling thread since the last reset that were folded into the node of a launch before them (libxsmm_hip_launch_count counts them too). */
LIBXSMM_API unsigned long long libxsmm_hip_fused_launch_count(int reset);
/** Sticky error state of the calling thread (0 = none); kernels have no error channel. */
LIBXSMM_API int libxsmm_hip_get_last_error(void);
LIBXSMM_API const char* libxsmm_hip_get_last_error_string(void);
LIBXSMM_API void libxsmm_hip_clear_last_error(void);

/* ---- device memory for C callers that do not want to include HIP headers ----------- */
LIBXSMM_API void* libxsmm_hip_malloc(size_t nbytes);
LIBXSMM_API void libxsmm_hip_free(void* device_ptr);
LIBXSMM_API int libxsmm_hip_memcpy_h2d(void* device_dst, const void* host_src, size_t nbytes);
LIBXSMM_API int libxsmm_hip_memcpy_d2h(void* host_dst, const void* device_src, size_t nbytes);
LIBXSMM_API int libxsmm_hip_memset(void* device_dst, int value, size_t nbytes);

/* ---- batched launches: the caller's loop moved into one grid ------------------------ */
LIBXSMM_API void libxsmm_hip_gemm_batch_strided(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param,
  size_t count, long long stride_a, long long stride_b, long long stride_c);
/** Adds byte strides for d.primary (fused bias) and c.secondary (ReLU bitmask). */
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_strided(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* param,
  size_t count, long long stride_a, long long stride_b, long long stride_c, long long stride_d, long long stride_mask);
/**
 * 2-D strided batch -- the two nested loops a caller runs to build a blocked GEMM out of (BR)GEMM tiles
 * [ref: the loop nests around the kernel in samples/xgemm/gemm_kernel.c:3186-3226 and the DL drivers built on BRGEMM]:
 *   for (j = 0; j < count_j; ++j) for (i = 0; i < count_i; ++i) { q = *p;
 *     q.a.primary = (char*)p->a.primary + i*stride_a_i;  q.b.primary = (char*)p->b.primary + j*stride_b_j;
 *     q.c.primary = (char*)p->c.primary + i*stride_c_i + j*stride_c_j;  f(&q); }
 * A is re-used by every j and B by every i: the launch deals contiguous bands of j to the eight XCDs so that the re-use
 * happens in their L2s.  The ext form steps d.primary (column bias) with i and c.secondary (ReLU bitmask) with both.
 * MXFP4 / MX scales step with their operand as in the 1-D form.
 */
LIBXSMM_API void libxsmm_hip_gemm_batch_strided_2d(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param, size_t count_i, size_t count_j,
  long long stride_a_i, long long stride_b_j, long long stride_c_i, long long stride_c_j);
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_strided_2d(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* param, size_t count_i, size_t count_j,
  long long stride_a_i, long long stride_b_j, long long stride_c_i, long long stride_c_j, long long stride_d_i, long long stride_mask_i, long long stride_mask_j);
/**
 * Pointer-list batch: element i uses a_list[i], b_list[i], c_list[i] as its `primary`
 * slots.  The three lists themselves must be device-accessible arrays of `count` pointers.
 */
LIBXSMM_API void libxsmm_hip_gemm_batch_pointers(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param,
  size_t count, const void* const* a_list, const void* const* b_list, void* const* c_list);
LIBXSMM_API void libxsmm_hip_meltw_unary_batch_strided(libxsmm_meltwfunction_unary kernel, const libxsmm_meltw_unary_param* param,
  size_t count, long long stride_in, long long stride_out, long long stride_aux);
LIBXSMM_API void libxsmm_hip_meltw_binary_batch_strided(libxsmm_meltwfunction_binary kernel, const libxsmm_meltw_binary_param* param,
  size_t count, long long stride_in0, long long stride_in1, long long stride_out);
LIBXSMM_API void libxsmm_hip_meltw_ternary_batch_strided(libxsmm_meltwfunction_ternary kernel, const libxsmm_meltw_ternary_param* param,
  size_t count, long long stride_in0, long long stride_in1, long long stride_in2, long long stride_out);
/**
 * Strided batch of a matrix equation: element i (0 <= i < count) is the call kernel(&q) where q = *param except
 *   q.inputs[k].primary   = (char*)param->inputs[k].primary   + i * stride_inputs[k]    (0 <= k < ninputs; 0 = shared: gamma, beta, eps, ...)
 *   q.output.primary      = (char*)param->output.primary      + i * stride_output
 *   q.output.secondary    = (char*)param->output.secondary    + i * stride_output_aux   (ReLU-bitmask / SCATTER-index head; unused otherwise)
 *   q.ops_args[k].primary = (char*)param->ops_args[k].primary + i * stride_ops_args[k]  (0 <= k < nops_args; DUMP destinations)
 * Everything else is shared by all elements: GATHER index lists (inputs[k].secondary), BRGEMM block counts (ops_args[k].tertiary) and scalar op
 * arguments such as LEAKY_RELU's alpha.  Elements run concurrently, so a buffer that the caller's loop re-uses (the DUMP scratch of a softmax)
 * needs a stride here.  Elements whose outputs overlap are undefined, as in the GEMM batches.  stride_ops_args may be NULL (all zero).
 * Follows the thread's launch mode: blocking (1 x 1 inputs / a 1 x 1 output may be host memory), stream-ordered, or coalescing (the queue is
 * flushed first).  Error -3: not an equation handle, or a non-zero stride on something shared; -2: ninputs below the equation's input positions.
 */
LIBXSMM_API void libxsmm_hip_meqn_batch_strided(libxsmm_meqn_function kernel, const libxsmm_meqn_param* param, size_t count,
  int ninputs, const long long* stride_inputs, long long stride_output, long long stride_output_aux,
  int nops_args, const long long* stride_ops_args);
/**
 * Accumulating strided batch of a matrix equation: the caller's loop whose every iteration reads AND writes the same output -- the dgamma / dbeta sums
 * of a layernorm backward pass [ref: samples/equation/equation_layernorm.c, tpp_layernorm_bwd_fp32: dgamma_func / dbeta_func inside the s2 loop]:
 *   libxsmm_hip_meqn_batch_strided_accumulate(kernel, param, count, ninputs, stride_inputs, nops_args, stride_ops_args, order)
 *     ==  for (i = 0; i < count; ++i) { q = *param;                      (in THIS order)
 *           q.inputs[k].primary   = (char*)param->inputs[k].primary   + i * stride_inputs[k];
 *           q.ops_args[k].primary = (char*)param->ops_args[k].primary + i * stride_ops_args[k];
 *           kernel(&q); }                                                (q.output is NOT stepped)
 * At least one input position of the tree must be the carried operand: inputs[k].primary == output.primary, stride_inputs[k] == 0, declared with the
 * output's m, n, ld and type.  Element i reads it as element i - 1 left it.  No other operand may overlap the output.  F32 and BF16 outputs.
 * order = LIBXSMM_HIP_MEQN_ORDER_LOOP: the result has the bits of the loop above -- every element's rounding in the loop's sequence (a BF16 output is
 * rounded to BF16 after every element).  Element-wise trees run as ONE launch (the elements are walked inside the kernel); trees with reductions or
 * GEMM nodes, misaligned operands and LIBXSMM_HIP_JIT=0 run the elements one after another through the single-call path.
 * order = LIBXSMM_HIP_MEQN_ORDER_ANY: the caller allows the sum over the elements to be re-associated.  It is a permission, not a request: it takes effect
 * for an F32 output whose head is output + x (BINARY_ADD, no broadcast) or output + x * y (TERNARY_MULADD, the output as in2) with the carried position
 * nowhere else in the tree, and only for the sizes where it is faster.  Then the element axis is cut into S contiguous slices,
 * S a function of (count, m, n) alone; slice s sums its elements [s * count / S, (s + 1) * count / S) in ascending order starting from +0, the S partial sums
 * are added in ascending slice order, and the output's original value is added last.  No atomics: the same bits in every run, on every stream.
 * Follows the thread's launch mode as libxsmm_hip_meqn_batch_strided does: blocking (per-element 1 x 1 inputs, e.g. arrays with stride 4, may be host
 * memory), stream-ordered, or coalescing (the queue is flushed first).  Errors are set before anything is launched.  -3: not an equation handle; no
 * carried operand; a carried operand whose shape, leading dimension or type differs from the output's; a head with a side channel (output.secondary:
 * ReLU bitmask, UNZIP, SCATTER); a DUMP destination with stride 0 while count > 1; a non-zero stride on something shared (as the strided entry); an unknown
 * order.  -2: fewer input strides than the equation's input positions.  count = 0 does nothing.  stride_ops_args may be NULL (all zero).
 */
#define LIBXSMM_HIP_MEQN_ORDER_LOOP 0   /* exactly the loop's sequence of roundings */
#define LIBXSMM_HIP_MEQN_ORDER_ANY  1   /* the caller allows the sum over elements to be re-associated */
LIBXSMM_API void libxsmm_hip_meqn_batch_strided_accumulate(libxsmm_meqn_function kernel, const libxsmm_meqn_param* param,
  size_t count, int ninputs, const long long* stride_inputs, int nops_args, const long long* stride_ops_args, int order);
/**
 * Grouped batch: several strided batches, each through its own (BR)GEMM handle and so of its own shape, in one call -- the caller that calls several
 * handles from its OpenMP region [ref: samples/xgemm/gemm_kernel.c:4063-4066]:
 *   libxsmm_hip_gemm_batch_grouped(groups, ngroups)
 *     ==  for (g = 0; g < ngroups; ++g)
 *           libxsmm_hip_gemm_batch_strided(groups[g].kernel, &groups[g].param, groups[g].count, groups[g].stride_a, groups[g].stride_b, groups[g].stride_c);
 * The caller declares that no group reads or writes what another group writes (the contract of a pipeline section); the elements of one group follow
 * libxsmm_hip_gemm_batch_strided.  Groups through plain or STRIDE batch-reduce handles of f32 x f32 -> f32 or bf16 x bf16 -> f32 / bf16 (A flat or VNNI_A,
 * B flat, C not VNNI, no transposes) leave as ONE launch per precision class, except f32 groups of 2048 work items (element x C tile) or more, which are
 * faster on their own kernels; a class with a single such group, and every other accepted handle (other types, transposes, ADDRESS /
 * OFFSET batch-reduce, bitmask-compressed A, packed sparse), runs as that group's own strided launch, in list order, on the same stream.  Follows the
 * thread's launch mode: blocking (returns when every group is done), stream-ordered (valid after libxsmm_hip_sync), coalescing (the queue is flushed
 * first), inside a pipeline section (the launches go to the section's lanes).  Operands must be device-accessible -- for groups of count 1 as well, where a
 * blocking libxsmm_hip_gemm_batch_strided call would still stage host-resident operands: the grouped launch reads them on the device as they are.  Every group is
 * validated before anything is launched.  Error -2: groups == NULL with ngroups > 0, a batch-reduce handle without op.tertiary; -3: an unknown, TPP /
 * equation or ext handle, or a call while the thread's stream is being captured into a graph (the group table lives for the call only).  count = 0 skips
 * a group.
 */
typedef struct libxsmm_hip_gemm_group {
  libxsmm_gemmfunction kernel;      /* any handle libxsmm_hip_gemm_batch_strided accepts (no ext handles) */
  libxsmm_gemm_param   param;       /* element 0 of the group; op.tertiary = batch-reduce count for BRGEMM handles */
  size_t               count;       /* elements of this group; 0 = skipped */
  long long            stride_a, stride_b, stride_c;   /* byte strides of the primary slots; 0 = shared (weights) */
} libxsmm_hip_gemm_group;
LIBXSMM_API void libxsmm_hip_gemm_batch_grouped(const libxsmm_hip_gemm_group* groups, size_t ngroups);
/**
 * Grouped batch through ext handles: a layer of several GEMM shapes, each followed by its bias and activation -- the reference's fused BRGEMM call
 * [ref: src/generator_gemm_reference_impl.c:294-372] issued from the caller's loop over shapes [ref: samples/xgemm/gemm_kernel.c:4063-4066]:
 *   libxsmm_hip_gemm_ext_batch_grouped(groups, ngroups)
 *     ==  for (g = 0; g < ngroups; ++g)
 *           libxsmm_hip_gemm_ext_batch_strided(groups[g].kernel, &groups[g].param, groups[g].count, groups[g].stride_a, groups[g].stride_b,
 *                                              groups[g].stride_c, groups[g].stride_d, groups[g].stride_mask);
 * The contract is that of libxsmm_hip_gemm_batch_grouped: the caller declares the groups independent, operands are device-accessible, every group is
 * validated before anything is launched, and the call follows the thread's launch mode (blocking, stream-ordered, coalescing -- flushed first --, pipeline
 * section).  Groups through ext handles of f32 x f32 -> f32 or bf16 x bf16 -> f32 / bf16 (plain or STRIDE batch-reduce, A flat or VNNI_A, B flat, C not VNNI,
 * NN, beta 0 or 1, the hints) with BINARY_ADD + BCAST_COL_IN_0/1, cp RELU (with or without BITMASK_2BYTEMULT) or cp SIGMOID leave as ONE launch per fused
 * precision class; ext handles without operators join the plain classes of libxsmm_hip_gemm_batch_grouped under its rule.  A fused f32 group of 2048 work
 * items (element x C tile) or more on 32 x 32 tiles (m or n above 16) whose m and n are multiples of 16 is faster on its own ext kernel and leaves, every other fused f32 group
 * stays (measured: DESIGN.md section 8.1); a class with a single group runs that group's own kernel.  Everything else libxsmm_hip_gemm_ext_batch_strided accepts (other
 * types, transposes, ADDRESS / OFFSET batch-reduce, a batch-reduce count of 0, 2^32 items or more) runs as that group's own ext strided launch, in list
 * order on the same stream, bit for bit what that call computes.
 * Per element of a fused group (the semantics of libxsmm_hip_gemm_ext_batch_reduce_segments for one C block): the bias has C's type; the accumulator starts
 * at bias[i], at bias[i] + C(i,j) (beta = 1, one f32 add), or at C(i,j) / +0 without a bias; one chain over (block, k); mask bit i % 8 of byte
 * i / 8 + j * (mask_ld / 8), mask_ld = ldc rounded up to 16, is !(x <= 0) of the sum and is written for i < m, j < n only; then the activation; then one
 * rounding for a bf16 C.  For f32 the result is the k-ordered fmaf chain started at the bias, bit for bit.
 * Error -2: groups == NULL with ngroups > 0, a batch-reduce handle without op.tertiary, a column-bias handle with param.d.primary NULL, a bitmask handle
 * with param.c.secondary NULL; -3: an unknown handle, a non-ext / TPP / equation / sparse handle (plain handles go to libxsmm_hip_gemm_batch_grouped), or a
 * call while the thread's stream is being captured (the tables live for the call only: make the list a plan, below); -4: no device.  count = 0 skips a
 * group; ngroups = 0 does nothing.
 */
typedef struct libxsmm_hip_gemm_ext_group {
  libxsmm_gemmfunction_ext kernel;  /* any handle libxsmm_hip_gemm_ext_batch_strided accepts */
  libxsmm_gemm_ext_param   param;   /* element 0; d.primary = bias, c.secondary = ReLU bitmask, op.tertiary = batch-reduce count */
  size_t                   count;   /* elements of this group; 0 = skipped */
  long long                stride_a, stride_b, stride_c, stride_d, stride_mask;   /* byte strides; 0 = shared */
} libxsmm_hip_gemm_ext_group;
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_grouped(const libxsmm_hip_gemm_ext_group* groups, size_t ngroups);
/**
 * Group plans: the group tables of a list built once and kept in device memory that the plan owns -- for the caller whose list is fixed (10 000 groups of
 * one problem: no validation, no table build and no upload per call) and for graph capture, which the two grouped calls refuse.
 *   plan = libxsmm_hip_gemm_group_plan_create(groups, ngroups)         (a list of libxsmm_hip_gemm_batch_grouped)
 *   plan = libxsmm_hip_gemm_ext_group_plan_create(groups, ngroups)     (a list of libxsmm_hip_gemm_ext_batch_grouped)
 *   libxsmm_hip_gemm_group_plan_launch(plan)    ==  the grouped call on the list given at create
 * Create validates with the codes of the call and applies its launch rule; the caller's arrays (the list, and the batch-reduce counts op.tertiary points
 * at: their VALUES are kept) may be freed afterwards.  A plan takes only groups of the kind that can enter the grouped kernels (the eligible handles
 * above); those that the launch rule sends to their own kernels (large f32 groups, a class with one group) run their own strided launch from a stored copy
 * of their param.  Any other group -- other types, transposes, ADDRESS / OFFSET batch-reduce, packed sparse, a count of 0 batch-reduce blocks -- is refused:
 * -3, NULL, the message names the group (such a launch may stage per-call host data, which a replayed graph cannot redo).  Create returns NULL with -4 when
 * there is no device, after validation.  A plan belongs to the device that is current at create.
 * Launch issues only kernel launches that read the resident tables, so it may be called while the thread's stream is being captured into a graph (in
 * stream-ordered mode, like every captured call).  The operand bases travel in the tables: a replay computes from what the operands hold then.  It follows
 * the thread's launch mode like the grouped calls.  -2: plan == NULL; -3: another device is current, or libxsmm_finalize released the plan's handles.
 * libxsmm_hip_gemm_group_plan_launches(plan): the kernel launches one launch issues (libxsmm_hip_launch_count).
 * Destroy waits for the thread's stream and frees the tables: a graph that captured a launch of the plan must not be replayed afterwards.  While the
 * thread's stream is being captured it is refused (-3) and the plan is kept.
 */
typedef struct libxsmm_hip_gemm_group_plan libxsmm_hip_gemm_group_plan;
LIBXSMM_API libxsmm_hip_gemm_group_plan* libxsmm_hip_gemm_group_plan_create(const libxsmm_hip_gemm_group* groups, size_t ngroups);
LIBXSMM_API libxsmm_hip_gemm_group_plan* libxsmm_hip_gemm_ext_group_plan_create(const libxsmm_hip_gemm_ext_group* groups, size_t ngroups);
LIBXSMM_API void libxsmm_hip_gemm_group_plan_launch(const libxsmm_hip_gemm_group_plan* plan);
LIBXSMM_API int libxsmm_hip_gemm_group_plan_launches(const libxsmm_hip_gemm_group_plan* plan);
LIBXSMM_API void libxsmm_hip_gemm_group_plan_destroy(libxsmm_hip_gemm_group_plan* plan);
/**
 * Segments: a batch of ADDRESS batch-reduce calls whose reduce count differs from call to call -- the count is the one argument the reference re-reads on
 * every call [ref: src/generator_gemm_reference_impl.c:490-492] -- as ONE launch: a block-sparse matrix times a dense one (one BRGEMM per block row of C),
 * a stack of small products accumulating into blocks of C, a convolution whose border pixels see fewer taps.  `kernel` is an ADDRESS batch-reduce handle
 * (libxsmm_dispatch_brgemm with LIBXSMM_GEMM_BATCH_REDUCE_ADDRESS):
 *   libxsmm_hip_gemm_batch_reduce_segments(kernel, param, nsegments, seg_ptr, a_list, b_list, c_list)
 *     ==  for (s = 0; s < nsegments; ++s) { q = *param; cnt = seg_ptr[s+1] - seg_ptr[s];
 *           q.a.primary = (void*)(a_list + seg_ptr[s]);  q.b.primary = (void*)(b_list + seg_ptr[s]);
 *           q.c.primary = c_list[s];  q.op.tertiary = &cnt;  kernel(&q); }
 * seg_ptr holds nsegments + 1 entries, CSR-style and non-decreasing; a_list and b_list hold seg_ptr[nsegments] block pointers each, c_list nsegments.  All
 * four arrays must be device-accessible, like the lists of libxsmm_hip_gemm_batch_pointers: nothing is staged or uploaded per call, so a caller whose
 * pattern is fixed pays nothing on the host beyond the launch, and the call may be captured into a graph.  param's primary slots and op.tertiary are
 * ignored.  Segments whose C blocks overlap are undefined; A and B blocks may be shared freely between products and segments.  Within a segment the
 * products are summed in list order: starting from C (beta = 1) or +0 they form one accumulator chain over (product, k), as in the reference; for f32 the
 * result is the k-ordered fmaf chain bit for bit.  A segment of count 0 is the reference's call with a count of 0: beta = 0 sets the m x n block to +0,
 * beta = 1 leaves it untouched.  Work is handed to the device in list order (a work item is a segment's C tile, taken up in ascending order): a caller who
 * lists long segments first gets longest-first scheduling for free; a segment is never split, which would reorder its sum.
 * Eligible handles: f32 x f32 -> f32, f64 x f64 -> f64, bf16 x bf16 -> f32 / bf16, F16 x F16 -> f32 / F16, BF8 x BF8 -> f32 / BF8, HF8 x HF8 -> f32 / HF8
 * (comp f32); A flat (or VNNI_A for bf16 and f16; for the 8-bit floats VNNI_A is required: A is taken as VNNI-4 only, A(i,k) at ((k / 4) * lda + i) * 4 + k % 4, k a multiple of 4), B flat,
 * C not VNNI, no transposes; beta 0 or 1; no flag beyond those and the hints; any m, n, k and leading dimensions whose element offsets inside an operand stay
 * below 2^31.  Block pointers need element alignment only (8-bit floats: any byte).
 * 8-bit floats (BF8 = E5M2, HF8 = E4M3) [ref: src/generator_gemm_reference_impl.c:2420-2510, own-type C :2511-2619]: per segment one f32 accumulator over
 * (product, k) in list order, started at +0 (beta = 0) or at C (beta = 1; an 8-bit C is widened to f32); an f32 C is stored as it is, an 8-bit C leaves through
 * the library's two-step conversion f32 -> f16 -> 8 bits, NaNs in software -- the conversion the dense 8-bit float kernels store with.  A count of 0 stores
 * beta * C (for an 8-bit C the round trip of the byte: the identity on every code that is not a NaN).  Bytes of C outside m x n stay the caller's.  The matrix
 * core (v_mfma_f32_32x32x16_{bf8_bf8,fp8_fp8}, v_mfma_f32_16x16x32_*) aligns the products of one instruction before it adds them, so the result is the
 * reference's serial chain within a tolerance -- bitwise where every partial sum is exact -- like the dense 8-bit float kernels.
 * IEEE halves (F16 x F16 -> f32 / F16, any comp type but F16; A flat or VNNI-2 -- the bf16 image --, B and C flat) follow the reference's F16 loop, which is
 * NOT the bf16 rule [ref: src/generator_gemm_reference_impl.c:2025-2124]: per element the sum is one f32 chain over (product, k) in list order STARTED AT +0
 * (v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x16_f16: the products, exact in f32, are added in the instruction's order -- bitwise the reference where every
 * partial sum is exact, within a tolerance otherwise); then, under beta = 1, C is ROUNDED TO A HALF, widened and added to the sum in one f32 add -- the
 * identity for an f16 C, a real rounding for an f32 C; then one store, an f32 C as it is, an f16 C through the hardware's round-to-nearest-even conversion.
 * A count of 0 under beta = 1 therefore stores f16(C) widened: for an f32 C NOT C's own bits, unlike every other class.  comp type F16 (the running sum
 * rounded to a half after every product) is refused with -3: only the dense generic kernel does that.  No f16 handle has TRANS_A (libxsmm_dispatch_brgemm
 * returns NULL, as the reference's F16 loop has no transposed A).
 * Follows the thread's launch mode: blocking (returns when done), stream-ordered, coalescing (the queue is flushed first),
 * inside a pipeline section (the launch goes to a lane).  Errors are set before anything is launched.  -2: param, seg_ptr, a_list, b_list or c_list is NULL
 * while nsegments > 0; -3: an unknown handle, a TPP / equation / sparse / ext handle, a GEMM handle that is not ADDRESS batch-reduce, or a type, layout or
 * flag outside the list above (the message names which); -4: no device.  nsegments = 0 does nothing.  libxsmm_hip_kernel_name(kernel, 1) names the
 * kernel that ran (gemm_segments_f32_kernel, _f64_kernel, _bf16_kernel, _f16_kernel, _bf8_kernel, _hf8_kernel).
 */
LIBXSMM_API void libxsmm_hip_gemm_batch_reduce_segments(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param,
  size_t nsegments, const unsigned long long* seg_ptr, const void* const* a_list, const void* const* b_list, void* const* c_list);

/* The segments call through an ext handle (libxsmm_dispatch_brgemm_ext with LIBXSMM_GEMM_BATCH_REDUCE_ADDRESS): the handle's column bias and activation are
 * applied per segment inside the one launch, as the reference's fused call applies them [ref: src/generator_gemm_reference_impl.c:294-372]:
 *   libxsmm_hip_gemm_ext_batch_reduce_segments(kernel, param, nsegments, seg_ptr, a_list, b_list, c_list, d_list, mask_list)
 *     ==  for (s = 0; s < nsegments; ++s) { q = *param; cnt = seg_ptr[s+1] - seg_ptr[s];
 *           q.a.primary = (void*)(a_list + seg_ptr[s]);  q.b.primary = (void*)(b_list + seg_ptr[s]);  q.c.primary = c_list[s];
 *           q.d.primary = d_list ? (void*)d_list[s] : param->d.primary;  q.c.secondary = mask_list ? mask_list[s] : NULL;
 *           q.op.tertiary = &cnt;  kernel(&q); }
 * seg_ptr, a_list, b_list and c_list are those of libxsmm_hip_gemm_batch_reduce_segments: device-accessible, read in place, nothing staged, capturable.
 * d_list holds nsegments pointers to the m-vector bias of C's type (entries may repeat; element alignment only); d_list == NULL on a handle with a column
 * bias means that param->d.primary -- device-accessible, passed by value in the kernel arguments -- is the bias of every segment.  mask_list holds nsegments
 * pointers to ReLU bitmask blocks of ((ldc + 15) / 16) * 16 / 8 * n bytes each; it is required exactly when the handle's ReLU carries
 * LIBXSMM_MELTW_FLAG_UNARY_BITMASK_2BYTEMULT and is ignored otherwise.  Overlapping C blocks or overlapping mask blocks are undefined.
 * Per segment: the accumulator starts at bias[i] (beta = 0), at bias[i] + C(i,j) (beta = 1, one f32 add), or at C(i,j) / +0 without a bias; one chain over
 * (product, k) in list order; mask bit i % 8 of byte i / 8 + j * (mask_ld / 8) is !(x <= 0) of the sum and is written for i < m, j < n only -- every other
 * bit and byte of the mask block stays the caller's; then the activation; then one rounding for a bf16 C.  A segment of count 0 is the reference's call with a
 * count of 0: it stores the activation of the start value (the bias, bias + C, C or +0) and the mask taken from it.
 * Eligible handles: ADDRESS batch-reduce ext handles under the plain entry's type, layout and flag rules (f32 -> f32, bf16 -> f32 / bf16; A flat or VNNI-2,
 * B flat, C not VNNI, NN; beta 0 or 1; the hints; element offsets below 2^31) with BINARY_ADD + BCAST_COL_IN_0/1, cp RELU (with or without bitmask), cp
 * SIGMOID, or no operator at all -- an ext handle without operators is taken for f64 and for the 8-bit floats (BF8 / HF8 -> f32 / own type, A VNNI-4) as well
 * and runs the plain kernels; an 8-bit float ext handle with a bias or an activation is refused ("taken without operators only").  F16 -> f32 / F16 ext
 * handles are taken with every operator of the list (gemm_segments_f16_fused_kernel), the bias having C's type, under the F16 rule of the plain entry
 * [ref: src/generator_gemm_reference_impl.c:296-317 with :2112-2117]: the sum runs from +0; the start value -- C, the bias, or bias + C in one f32 add -- is
 * rounded to a half, widened and added behind it; then mask, activation and store.  A segment of count 0 stores the activation of f16(start).  Errors are set before
 * anything is launched.  -2: param, seg_ptr, a_list, b_list or c_list is NULL while nsegments > 0; a bias handle with d_list and param->d.primary both NULL; a bitmask
 * handle with mask_list NULL.  -3: an unknown handle, a non-ext / TPP / equation / sparse handle, a handle that is not ADDRESS batch-reduce, a type, layout,
 * flag or operator outside the list (the message names which).  -4: no device.  nsegments = 0 does nothing.  Follows the thread's launch mode like the plain
 * entry.  libxsmm_hip_kernel_name(kernel, 1) names the kernel that ran (gemm_segments_f32_fused_kernel, gemm_segments_bf16_fused_kernel; without operators
 * the plain entry's kernels).
 */
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_reduce_segments(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* param,
  size_t nsegments, const unsigned long long* seg_ptr, const void* const* a_list, const void* const* b_list, void* const* c_list,
  const void* const* d_list, void* const* mask_list);

/* Segments through an OFFSET batch-reduce handle (libxsmm_dispatch_brgemm with LIBXSMM_GEMM_BATCH_REDUCE_OFFSET), with transposed operands accepted: the
 * forward AND the backward passes of a block-sparse layer as one launch each -- Y = W X (NN), dX = W^T dY (LIBXSMM_GEMM_FLAG_TRANS_A, the lists in block-column
 * order over the same W buffer), dW_b = sum_n dY_n X_n^T (LIBXSMM_GEMM_FLAG_TRANS_B) -- from lists that do not depend on where the operands lie
 * [ref: src/generator_gemm_reference_impl.c:509-513, :186-188]:
 *   libxsmm_hip_gemm_batch_reduce_segments_offsets(kernel, param, nsegments, seg_ptr, a_offs, b_offs, c_offs)
 *     ==  for (s = 0; s < nsegments; ++s) { q = *param; cnt = seg_ptr[s+1] - seg_ptr[s];
 *           q.a.secondary = (void*)(a_offs + seg_ptr[s]);  q.b.secondary = (void*)(b_offs + seg_ptr[s]);
 *           q.c.primary   = (char*)param->c.primary + c_offs[s];  q.op.tertiary = &cnt;  kernel(&q); }
 * param->a.primary, b.primary and c.primary are the three bases: device-accessible, and passed BY VALUE in the kernel arguments -- a call captured into a
 * graph replays on the same three bases (overwrite the operands in place, or capture one call per buffer).  seg_ptr holds nsegments + 1 entries, CSR-style
 * and non-decreasing; a_offs and b_offs hold seg_ptr[nsegments] signed byte offsets each, c_offs nsegments.  All four arrays must be device-accessible and are
 * read in place: nothing is staged or uploaded, so the call may be captured, and a caller whose pattern is fixed computes the lists once and only moves the
 * bases -- another layer's activations, dY instead of X, the other half of a double buffer.  param's other slots are ignored.  Segments whose C blocks overlap
 * are undefined; A and B blocks may be shared freely.  Order, start value and count 0 are those of libxsmm_hip_gemm_batch_reduce_segments: one accumulator
 * chain over (product, k) in list order from C (beta = 1) or +0; a segment of count 0 stores beta * C; for f32 the result is the k-ordered fmaf chain bit for
 * bit, in every form.  Work is handed out in list order; a segment is never split.
 * Eligible handles: f32 x f32 -> f32, f64 x f64 -> f64, bf16 x bf16 -> f32 / bf16; BF8 x BF8 -> f32 / BF8 and HF8 x HF8 -> f32 / HF8 NN only, A VNNI-4
 * (LIBXSMM_GEMM_FLAG_VNNI_A required, TRANS_A / TRANS_B refused), with the semantics given at libxsmm_hip_gemm_batch_reduce_segments; F16 x F16 -> f32 / F16
 * (comp type not F16) NN and NT, A flat or VNNI-2, with the F16 rule given there (the sum from +0, f16(C) added behind it; a count of 0 under beta = 1 stores
 * f16(C) widened) -- no f16 handle with TRANS_A exists, so TN / TT cannot be asked for (gemm_segments_offs_f16_kernel<0,tb>).  A flat, A with TRANS_A (flat, A(i,k) at i * lda + k, lda >= k) or, for
 * bf16, VNNI-2 without TRANS_A; B flat or B with TRANS_B (flat, B(k,j) at k * ldb + j, ldb >= n); both transposes together are allowed; VNNI_B and VNNI_C are
 * refused; beta 0 or 1; no flag beyond those and the hints; element offsets inside one operand (lda * m and ldb * k for transposed ones) stay below 2^31.
 * Offsets need element alignment only.  Follows the thread's launch mode: blocking, stream-ordered, coalescing (the queue is flushed first), inside a pipeline
 * section.  Errors are set before anything is launched, one per refusal.  -2: param, seg_ptr, a_offs, b_offs, c_offs or one of the three bases is NULL while
 * nsegments > 0; -3: an unknown handle, a TPP / equation / sparse / ext handle, a GEMM handle that is not OFFSET batch-reduce, or a type, layout or flag
 * outside the list above (the message names which); -4: no device.  nsegments = 0 does nothing.  libxsmm_hip_kernel_name(kernel, 1) names the kernel that
 * ran (gemm_segments_offs_f32_kernel<ta,tb>, _f64_kernel<ta,tb>, _bf16_kernel<ta,tb>: one instance per pair of transposes; gemm_segments_offs_bf8_kernel<0,0>,
 * gemm_segments_offs_hf8_kernel<0,0>).  The two ADDRESS entries above keep refusing transposed operands; ext handles go to
 * libxsmm_hip_gemm_ext_batch_reduce_segments_offsets below.
 */
LIBXSMM_API void libxsmm_hip_gemm_batch_reduce_segments_offsets(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param,
  size_t nsegments, const unsigned long long* seg_ptr, const long long* a_offs, const long long* b_offs, const long long* c_offs);

/* OFFSET segments through an ext handle (libxsmm_dispatch_brgemm_ext with LIBXSMM_GEMM_BATCH_REDUCE_OFFSET): the call a convolution or a block-sparse layer in
 * the reference's style makes -- offset lists computed once per layer geometry, bias and activation fused -- with a count of its own per C block, as ONE launch
 * [ref: src/generator_gemm_reference_impl.c:509-513, :186-188 for the offsets, src/generator_gemm_reference_impl.c:294-372 for the epilogue]:
 *   libxsmm_hip_gemm_ext_batch_reduce_segments_offsets(kernel, param, nsegments, seg_ptr, a_offs, b_offs, c_offs, d_offs, mask_offs)
 *     ==  for (s = 0; s < nsegments; ++s) { q = *param; cnt = seg_ptr[s+1] - seg_ptr[s];
 *           q.a.secondary = (void*)(a_offs + seg_ptr[s]);  q.b.secondary = (void*)(b_offs + seg_ptr[s]);
 *           q.c.primary   = (char*)param->c.primary + c_offs[s];
 *           q.d.primary   = (char*)param->d.primary + (d_offs ? d_offs[s] : 0);
 *           q.c.secondary = mask_offs ? (char*)param->c.secondary + mask_offs[s] : NULL;
 *           q.op.tertiary = &cnt;  kernel(&q); }
 * Five bases, all device-accessible and passed BY VALUE in the kernel arguments: param->a.primary, b.primary and c.primary as in
 * libxsmm_hip_gemm_batch_reduce_segments_offsets; param->d.primary, the bias base, needed only when the handle has a column bias; param->c.secondary, the mask
 * base, needed only with LIBXSMM_MELTW_FLAG_UNARY_BITMASK_2BYTEMULT.  seg_ptr, a_offs, b_offs and c_offs are those of the plain offsets entry.  d_offs and
 * mask_offs hold nsegments signed byte offsets each: d_offs[s] leads to the m-vector bias of C's type (entries may repeat; element alignment only), and
 * d_offs == NULL on a bias handle means that the one bias at param->d.primary serves every segment; mask_offs[s] leads to a ReLU bitmask block of
 * ((ldc + 15) / 16) * 16 / 8 * n bytes, is required exactly when the handle's ReLU carries the bitmask flag and is ignored otherwise.  Every list is read in
 * place on the device: nothing is staged, the call may be captured, and a captured call replays on the same five bases.  Overlapping C blocks or overlapping
 * mask blocks are undefined; A, B and bias blocks may be shared freely.
 * Per segment, as in libxsmm_hip_gemm_ext_batch_reduce_segments: the accumulator starts at bias[i] (beta = 0), at bias[i] + C(i,j) (beta = 1, one f32 add), or
 * at C(i,j) / +0 without a bias; one chain over (product, k) in list order -- for f32 the k-ordered fmaf chain bit for bit in all four forms; mask bit i % 8 of
 * byte i / 8 + j * (mask_ld / 8) is !(x <= 0) of the sum and is written for i < m, j < n only -- every other bit and byte of the mask block stays the caller's;
 * then the activation; then one rounding for a bf16 C.  A segment of count 0 stores the activation of its start value (the bias, bias + C, C or +0) and the
 * mask taken from it.  Work is handed out in list order; a segment is never split.
 * Eligible handles: every handle the plain offsets entry takes, made into an ext handle -- f32 -> f32, bf16 -> f32 / bf16; A flat, TRANS_A or (bf16, without
 * TRANS_A) VNNI-2; B flat or TRANS_B; NN, TN, NT and TT; beta 0 or 1; the hints; element offsets below 2^31 -- with BINARY_ADD + BCAST_COL_IN_0/1, cp RELU (with
 * or without bitmask), cp SIGMOID, or no operator at all: an ext handle without operators is taken for f64 as well and runs the plain offsets kernels; f64 with
 * operators is refused; the same holds for the 8-bit floats (NN, A VNNI-4: without operators the plain offsets kernels, with operators refused).  F16 -> f32 /
 * F16 ext handles (NN, NT) are taken with every operator, under the F16 rule of libxsmm_hip_gemm_ext_batch_reduce_segments: the start value is rounded to a
 * half and added behind the sum (gemm_segments_offs_f16_fused_kernel<0,tb>).  Errors are
 * set before anything is launched, one per refusal.  -2: param, seg_ptr, a_offs, b_offs, c_offs or one of the three bases is
 * NULL while nsegments > 0; a bias handle with param->d.primary NULL; a bitmask handle with mask_offs or param->c.secondary NULL.  -3: an unknown handle, a
 * non-ext / TPP / equation / sparse handle, a handle that is not OFFSET batch-reduce, a type, layout, flag or operator outside the list (the message names
 * which).  -4: no device.  nsegments = 0 does nothing.  Follows the thread's launch mode like its siblings: blocking, stream-ordered, coalescing (the queue is
 * flushed first), inside a pipeline section.  libxsmm_hip_kernel_name(kernel, 1) names the kernel that ran (gemm_segments_offs_f32_fused_kernel<ta,tb>,
 * gemm_segments_offs_bf16_fused_kernel<ta,tb>; without operators the plain offsets entry's kernels).
 */
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_reduce_segments_offsets(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* param,
  size_t nsegments, const unsigned long long* seg_ptr, const long long* a_offs, const long long* b_offs, const long long* c_offs,
  const long long* d_offs, const long long* mask_offs);

/* Sliced segments: the two plain entries above with chains the CALLER has cut, so that several waves walk one long chain -- and still the same bits on every
 * run, stream and grid size.  The entries above never split a segment, because that would reorder its sum; here the caller says where a chain may be cut, and
 * the result is a pure function of the arguments (no atomics, no arrival order), as LIBXSMM_HIP_MEQN_ORDER_ANY of libxsmm_hip_meqn_batch_strided_accumulate is.
 *   libxsmm_hip_gemm_batch_reduce_segments_sliced(kernel, param, nblocks, blk_ptr, nslices, seg_ptr, a_list, b_list, c_list, workspace, workspace_bytes)
 *   libxsmm_hip_gemm_batch_reduce_segments_offsets_sliced(kernel, param, nblocks, blk_ptr, nslices, seg_ptr, a_offs, b_offs, c_offs, workspace, workspace_bytes)
 * A two-level CSR; a SLICE is what a segment is in the unsliced entries.  Slice j owns the products seg_ptr[j] .. seg_ptr[j+1] of a_list / b_list (a_offs /
 * b_offs); C block b owns the slices blk_ptr[b] .. blk_ptr[b+1].  blk_ptr has nblocks + 1 non-decreasing entries, blk_ptr[0] = 0, blk_ptr[nblocks] = nslices;
 * seg_ptr has nslices + 1 entries; c_list / c_offs has nblocks.  Every list is device-accessible and read in place: nothing is staged or uploaded, both calls
 * can be captured into a graph.  The ADDRESS form ignores param's primary slots; the OFFSET form takes the three bases from param->{a,b,c}.primary BY VALUE,
 * as its unsliced sibling does [ref: src/generator_gemm_reference_impl.c:509-513, :186-188].
 * Per block b:  P_j = one accumulator chain over (product, k), in list order, over slice j, STARTED AT +0, in the accumulator type (f32 for f32 and bf16
 * handles, f64 for f64) -- for f32 the k-ordered fmaf chain bit for bit, in every transpose form; an empty slice gives +0.  acc = C(i,j) widened to the
 * accumulator type (beta = 1) or +0 (beta = 0); for j ascending over the block's slices acc = acc + P_j, each one IEEE add in the accumulator type with
 * denormals kept; acc is stored with one rounding through the library's bf16 conversion for a bf16 C.  Bytes of the C block outside m x n stay the caller's.
 * 8-bit float handles (BF8 / HF8, A VNNI-4, NN): the partials are f32, started at +0; pass 2 adds them in ascending slice order to C widened to f32 or to +0
 * and stores once -- an f32 C as it is, an 8-bit C through the two-step conversion of the unsliced entries; the workspace holds 4-byte accumulators.
 * F16 handles: the partials are f32 from +0 (4-byte accumulators); pass 2 is acc = +0, acc += P_j in ascending slice order, THEN acc += f16(C) widened
 * (beta = 1), then one store (gemm_segments_slice_reduce_kernel<5> for an f16 C, <6> for an f32 C under beta = 1, <0> under beta = 0).  The start value comes
 * last here and in the unsliced entries, so for f16 one slice per block is bitwise the unsliced call FOR EVERY BETA.  A block without slices keeps the rule
 * below: under beta = 1 it is untouched, so an f32 C is not rounded there.
 * A block with no slices: beta = 0 stores +0, beta = 1 leaves the block untouched.  Consequences: with beta = 0 and one slice per block the result is bitwise
 * the unsliced call's (a chain started at +0 never yields -0, so +0 + P is P); with beta = 1 the original C is ADDED TO the first partial, not used as the
 * chain's start -- the documented difference from the unsliced entries, as in ORDER_ANY.  Blocks whose C overlaps are undefined; A and B blocks may be shared.
 * Meant for FEW blocks with LONG chains (the weight gradient of a block-sparse layer, dW_b = sum_n dY_n X_n^T with TRANS_B: hundreds of blocks, hundreds of
 * products each) and for the long tail of a skewed list; NOT for many short chains, where the second launch and the partials' round trip through memory are
 * pure overhead (DESIGN.md section 9.5 has the measurements).  The library chooses no slice lengths.
 * The workspace is the caller's: it holds the slice partials, its layout is the library's business and its contents after the call are unspecified.
 *   libxsmm_hip_gemm_batch_reduce_segments_sliced_workspace(kernel, nslices)
 * is the only authority on its size: a multiple of 16, 0 for nslices = 0, at least nslices * m * n * sizeof(acc) and at most nslices * the tile-padded block;
 * 0 with the handle's refusal code set for an ineligible handle (it serves both forms).  `workspace` must be 16-byte aligned and device-accessible,
 * workspace_bytes at least the query's value; nothing beyond that value is written.
 * Eligible handles: exactly those of libxsmm_hip_gemm_batch_reduce_segments (ADDRESS form) and of libxsmm_hip_gemm_batch_reduce_segments_offsets (OFFSET form,
 * with TRANS_A / TRANS_B under its rules).  Ext handles are refused here: they go to the two libxsmm_hip_gemm_ext_batch_reduce_segments*_sliced entries below.  Errors are set before anything is
 * launched, one per refusal.  -2: param, blk_ptr, c_list / c_offs or an OFFSET base is NULL while nblocks > 0; seg_ptr, a_*, b_* or workspace is NULL while
 * nslices > 0; workspace_bytes below the query's value.  -3: every handle refusal of the sibling entry, in its words; a workspace that is not 16-byte
 * aligned.  -4: no device.  nblocks = 0 does nothing.  Follows the thread's launch mode like the siblings (blocking, stream-ordered, coalescing: flushed
 * first, pipeline section).  A call is TWO kernel launches in order on the same stream or the same pipeline lane -- the slices' partials, then the blocks'
 * sums (gemm_segments_slice_reduce_kernel<cls>); with nslices = 0 the first is skipped.  libxsmm_hip_launch_count counts both;
 * libxsmm_hip_kernel_name(kernel, 1) names the first (gemm_segments_sliced_f32_kernel, _bf16_kernel, _f64_kernel, _bf8_kernel, _hf8_kernel;
 * gemm_segments_offs_sliced_f32_kernel<ta,tb>, _bf16_kernel<ta,tb>, _f64_kernel<ta,tb>, gemm_segments_offs_sliced_bf8_kernel<0,0>, _hf8_kernel<0,0>); the
 * second is gemm_segments_slice_reduce_kernel<0> for an f32 C, <1> bf16, <2> f64, <3> BF8, <4> HF8.
 */
LIBXSMM_API size_t libxsmm_hip_gemm_batch_reduce_segments_sliced_workspace(libxsmm_gemmfunction kernel, size_t nslices);
LIBXSMM_API void libxsmm_hip_gemm_batch_reduce_segments_sliced(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param,
  size_t nblocks, const unsigned long long* blk_ptr,
  size_t nslices, const unsigned long long* seg_ptr, const void* const* a_list, const void* const* b_list, void* const* c_list,
  void* workspace, size_t workspace_bytes);
LIBXSMM_API void libxsmm_hip_gemm_batch_reduce_segments_offsets_sliced(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* param,
  size_t nblocks, const unsigned long long* blk_ptr,
  size_t nslices, const unsigned long long* seg_ptr, const long long* a_offs, const long long* b_offs, const long long* c_offs,
  void* workspace, size_t workspace_bytes);

/* Sliced segments through an ext handle: the two sliced entries above with the fused epilogue of libxsmm_hip_gemm_ext_batch_reduce_segments /
 * ..._ext_batch_reduce_segments_offsets -- column bias, ReLU (+ bitmask), sigmoid -- applied to the blocks' sums in the second launch.  The call a small-batch
 * convolution or a skewed block-sparse layer makes: offset lists computed once per geometry, chains cut by the caller, bias and activation fused.
 *   libxsmm_hip_gemm_ext_batch_reduce_segments_sliced(kernel, param, nblocks, blk_ptr, nslices, seg_ptr, a_list, b_list, c_list, d_list, mask_list,
 *                                                     workspace, workspace_bytes)
 *   libxsmm_hip_gemm_ext_batch_reduce_segments_offsets_sliced(kernel, param, nblocks, blk_ptr, nslices, seg_ptr, a_offs, b_offs, c_offs, d_offs, mask_offs,
 *                                                             workspace, workspace_bytes)
 * The two-level CSR, the workspace contract and the base / list rules are those of the plain sliced entries.  d_list / d_offs and mask_list / mask_offs hold
 * NBLOCKS entries and mean what they mean in the unsliced ext entries: d_list == NULL (d_offs == NULL) on a bias handle says that the one bias at
 * param->d.primary serves every block; the mask list is required exactly when the ReLU carries LIBXSMM_MELTW_FLAG_UNARY_BITMASK_2BYTEMULT and is ignored
 * otherwise; bias entries need element alignment only, mask entries byte alignment only.  In the OFFSET form the five bases (param->{a,b,c,d}.primary and
 * param->c.secondary) travel BY VALUE.  Every list is read in place, nothing is staged: both calls can be captured into a graph.
 * Per C block b:
 *   partials     P_j = slice j's accumulator chain over (product, k) in list order, started at +0 in f32 -- what the plain sliced entries compute; an empty
 *                slice gives +0.
 *   start value  that of the unsliced ext entries: bias[i] (bias, beta = 0); bias[i] + C(i,j) (bias, beta = 1: ONE f32 add of the widened values);
 *                C(i,j) (beta = 1, no bias); +0 otherwise.
 *   sum          acc = start; for j ascending over the block's slices acc = acc + P_j, one IEEE f32 add each with denormals kept.
 *   mask         bit i % 8 of byte i / 8 + j * (mask_ld / 8), mask_ld = ldc rounded up to 16, is !(acc <= 0); written for i < m, j < n only -- every other bit
 *                and byte of the mask block stays the caller's.
 *   activation   ReLU (x <= 0 ? +0 : x) or the library's sigmoid, the functions of every fused kernel; then one store with C's ldc and type, with one rounding
 *                through the library's bf16 conversion for a bf16 C.  Bytes of C outside m x n stay the caller's.
 *   no slices    the block stores the activation of its start value and the mask taken from it, for EVERY beta: bitwise what the unsliced ext entry stores for a
 *                segment of count 0.
 * Consequences: with beta = 0, no bias and one slice per block the result is bitwise the unsliced ext call's for every activation, mask included (a chain
 * started at +0 never yields -0, so +0 + P is P); with a bias or beta = 1 the start value is ADDED TO the partial sum instead of starting the chain -- the
 * documented difference, as in the plain sliced entries.  No atomics, no arrival order: the same bits on every run, stream and grid size.  Overlapping C or
 * mask blocks are undefined; A, B and bias blocks may be shared.
 *   libxsmm_hip_gemm_ext_batch_reduce_segments_sliced_workspace(kernel, nslices)
 * is the only authority on the workspace's size for ext handles, with the bounds of the plain query; 0 with the refusal code set for an ineligible handle (an
 * operator outside the list among them).  The plain query keeps refusing ext handles.
 * Eligible handles: ADDRESS form, exactly those of libxsmm_hip_gemm_ext_batch_reduce_segments; OFFSET form, exactly those of
 * libxsmm_hip_gemm_ext_batch_reduce_segments_offsets (NN, TN, NT, TT).  An ext handle WITHOUT operators runs the plain sliced path unchanged and is bit for
 * bit the plain sliced call on the matching plain handle -- f64 included, and a block without slices under beta = 1 stays untouched; f64 with operators is
 * refused; plain handles are refused ("not an ext kernel").  Errors are set before anything is launched, one per refusal, with the siblings' codes and words:
 * -2 for a NULL argument that is needed (as in the plain sliced entries), a workspace below the query's value, a bias handle without a bias source (ADDRESS:
 * d_list and param->d.primary both NULL; OFFSET: param->d.primary NULL), a bitmask handle without mask_list / mask_offs or, OFFSET, without
 * param->c.secondary; -3 for every handle refusal and a workspace that is not 16-byte aligned; -4: no device.  nblocks = 0 does nothing.  Follows the thread's
 * launch mode like the siblings.  A call is TWO launches in order on one stream or pipeline lane (with nslices = 0 the first is skipped);
 * libxsmm_hip_launch_count counts both; libxsmm_hip_kernel_name(kernel, 1) names the first, the plain sliced entries' kernels, reused as they are; the second
 * is gemm_segments_slice_reduce_fused_kernel<0> (f32 C) or <1> (bf16 C).  DESIGN.md section 9.6 has the mask scheme and the measurements.
 * F16 -> f32 / F16 ext handles (pass 2: instances <5> for an f16 C, <6> for an f32 C) take the start value LAST, as their unsliced entries do: acc = +0;
 * acc += P_j ascending; then the start value -- C, the bias of C's type, or bias + C in one f32 add --, rounded to a half and widened, is added in one f32
 * add (nothing without a start); then mask, activation, store.  So one slice per block is bitwise the unsliced ext call for every beta and with a bias --
 * for the other classes only under beta = 0 without a bias -- and a block without slices is the unsliced segment of count 0.
 */
LIBXSMM_API size_t libxsmm_hip_gemm_ext_batch_reduce_segments_sliced_workspace(libxsmm_gemmfunction_ext kernel, size_t nslices);
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_reduce_segments_sliced(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* param,
  size_t nblocks, const unsigned long long* blk_ptr,
  size_t nslices, const unsigned long long* seg_ptr, const void* const* a_list, const void* const* b_list, void* const* c_list,
  const void* const* d_list, void* const* mask_list, void* workspace, size_t workspace_bytes);
LIBXSMM_API void libxsmm_hip_gemm_ext_batch_reduce_segments_offsets_sliced(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* param,
  size_t nblocks, const unsigned long long* blk_ptr,
  size_t nslices, const unsigned long long* seg_ptr, const long long* a_offs, const long long* b_offs, const long long* c_offs,
  const long long* d_offs, const long long* mask_offs, void* workspace, size_t workspace_bytes);

/* ---- multi-GPU: the batch / packed / N axis is split by contiguous blocks -----------
 * One process per GPU; no collective on the data path.  Rank r of `world` owns
 * [begin, end) of a `count`-long axis (first `count % world` ranks get one extra unit),
 * after rounding shard boundaries to `granule` units (e.g. the packed width's lane tile). */
LIBXSMM_API void libxsmm_hip_shard_range(size_t count, size_t granule, int world, int rank, size_t* begin, size_t* end);

/* ---- multi-GPU from ONE process and ONE host thread (C / C++ hosts: no launcher, no Python) ---------------------------------------
 * The reference scales out through the caller's loop over independent problems [ref: samples/xgemm/gemm_kernel.c:4063-4066,
 * samples/xgemm_sparse_Ainregs/pyfr_driver_asp_reg.c:379-393]; here that loop is cut into one contiguous block per device.
 * A shard = what ONE device does: a kernel handle, the param struct whose pointers name operands RESIDENT ON THAT DEVICE (the first
 * problem of the shard), and either count = 0 (one plain call kernel(param): the P / m_blocks / N splits, where every shard has a
 * handle of its own shape) or count > 0 (a strided batch exactly as libxsmm_hip_gemm[_ext]_batch_strided / libxsmm_hip_meltw_*_batch_strided:
 * stride[] = {a, b, c, d, mask} for (BR)GEMM and packed sparse handles, {in, out, aux} / {in0, in1, out} / {in0, in1, in2, out} for TPPs).
 * libxsmm_hip_launch_shards issues every shard on a stream of its own on the shard's device -- shards overlap, also several on one
 * device -- each with private staging scratch and partial-result workspaces, and (gather_bytes > 0) follows the shard's kernel with ONE
 * copy of gather_bytes from gather_src to gather_dst + gather_dst_offset on gather_device: the source device pushes over its own xGMI
 * link (hipMemcpyPeerAsync), so nshards - 1 links feed the root at once where a ring would be bound by one link per hop.
 * Blocking thread (default): returns when every shard and copy has finished.  Stream-ordered thread (libxsmm_hip_set_stream / _set_async):
 * the shards start behind what the thread's stream holds and the thread's stream continues behind them; libxsmm_hip_sync() waits.
 * Dense dispatch handles run on every device; created sparse kernels (pattern arrays, generated code) belong to the device that was
 * current at creation (libxsmm_hip_set_device) -- create one per device.  Operands must be device memory.  Returns EXIT_SUCCESS / EXIT_FAILURE
 * (libxsmm_hip_get_last_error_string says why). */
typedef struct libxsmm_hip_shard {
  int device;                          /* HIP device that holds this shard's operands */
  const void* kernel;                  /* any libxsmm_*function handle */
  const void* param;                   /* the matching param struct; its pointers are the shard's FIRST problem, in `device`'s memory */
  size_t count;                        /* 0: kernel(param) once;  > 0: strided batch of `count` problems */
  long long stride[5];                 /* byte strides of the batch (kind specific, see above) */
  const void* gather_src;              /* optional result gather: after the kernel, gather_bytes from here ... */
  size_t gather_bytes, gather_dst_offset;   /* ... to gather_dst + gather_dst_offset on gather_device */
  size_t gather_rows, gather_src_pitch, gather_dst_pitch;   /* gather_rows > 1 (round 6): a PITCHED gather -- gather_rows rows of gather_bytes each, the source rows
                                          gather_src_pitch bytes apart, the destination rows gather_dst_pitch: a shard's column block of a row-major result (the P
                                          axis of a packed C, the N axis of an FsSpMDM C) lands in place inside the whole result.  0 / 1: one contiguous copy. */
} libxsmm_hip_shard;
LIBXSMM_API int libxsmm_hip_launch_shards(const libxsmm_hip_shard* shards, int nshards, int gather_device, void* gather_dst);
/** The batch axis cut by libxsmm_hip_shard_range(count, 1, nshards, s): shard s owns problems [begin_s, end_s) and runs on devices[s]
 * (NULL: device s % device_count; a device may appear more than once).  shard_params[s] holds the pointers of problem begin_s in that device's
 * memory (every device holds only its own block of A / B / C; a shared operand -- stride 0 -- is replicated by the caller).
 * gather_dst != NULL: C of all shards is assembled at gather_dst + begin_s * stride_c on gather_device. */
LIBXSMM_API int libxsmm_hip_gemm_batch_strided_sharded(libxsmm_gemmfunction kernel, const libxsmm_gemm_param* shard_params, size_t count,
  long long stride_a, long long stride_b, long long stride_c, int nshards, const int* devices, int gather_device, void* gather_dst);
LIBXSMM_API int libxsmm_hip_gemm_ext_batch_strided_sharded(libxsmm_gemmfunction_ext kernel, const libxsmm_gemm_ext_param* shard_params, size_t count,
  long long stride_a, long long stride_b, long long stride_c, long long stride_d, long long stride_mask, int nshards, const int* devices, int gather_device, void* gather_dst);

/* ---- created (sparse) kernels, sharded (round 6) ---------------------------------------------------------------------------------------
 * Created kernels belong to the device they were created on (pattern arrays, generated code), so a C host that splits P / M-blocks / N over several GPUs
 * needs one handle per device.  These calls do that loop: given the creator's own arguments they cut the parallel axis with libxsmm_hip_shard_range
 * (granule = whole lane tiles), create one kernel per non-empty shard ON that shard's device (devices[s], NULL: s % device_count; a device may appear
 * several times -- virtual shards), and keep them together.  Every shard's operands live on its device in the shard's OWN compact layout:
 *   packed CSR / CSC (axis = the packed width P):   B [K][N][P_s], C [M][N][P_s] (CSR, A sparse);  A [M][K][P_s], C [M][N][P_s] (CSC, B sparse)
 *                                                    -- compact only: NULL unless ldc == n and ldb == n (A sparse) or lda == k (B sparse)
 *   BCSC (axis = the M-blocks = shape.m, as the creator takes them): A and C of the shard's M-blocks; the block-sparse B is replicated by the caller
 *   FsSpMDM (axis = N):                              B [K][N_s], C [M][N_s]  (leading dimensions = N_s)
 * libxsmm_hip_sharded_launch: shard_params[i] (i = 0 .. shards - 1, non-empty shards in order) holds shard i's operand pointers exactly as the plain kernel
 * takes them (FsSpMDM: b.primary, c.primary); all shards are issued by libxsmm_hip_launch_shards (one stream per shard, overlapping).  gather_dst != NULL
 * assembles C on gather_device: gather_dst_pitch = 0 places the shards' C blocks back to back (a valid packed layout of independent slabs),
 * gather_dst_pitch > 0 is the byte pitch of one row of the WHOLE result (P * elem for packed C, ldc * elem for FsSpMDM) and every shard's columns land in
 * place (BCSC: C of an M-block is contiguous, the pitch is ignored).  Returns EXIT_SUCCESS / EXIT_FAILURE like libxsmm_hip_launch_shards. */
typedef struct libxsmm_hip_sharded_kernel libxsmm_hip_sharded_kernel;
LIBXSMM_API libxsmm_hip_sharded_kernel* libxsmm_hip_create_packed_spgemm_csr_sharded(libxsmm_gemm_shape gemm_shape, libxsmm_bitfield gemm_flags, libxsmm_bitfield prefetch_flags,
  libxsmm_blasint packed_width, const unsigned int* row_ptr, const unsigned int* column_idx, const void* values, int nshards, const int* devices);
LIBXSMM_API libxsmm_hip_sharded_kernel* libxsmm_hip_create_packed_spgemm_csc_sharded(libxsmm_gemm_shape gemm_shape, libxsmm_bitfield gemm_flags, libxsmm_bitfield prefetch_flags,
  libxsmm_blasint packed_width, const unsigned int* column_ptr, const unsigned int* row_idx, const void* values, int nshards, const int* devices);
LIBXSMM_API libxsmm_hip_sharded_kernel* libxsmm_hip_create_packed_spgemm_bcsc_sharded(libxsmm_gemm_shape gemm_shape, libxsmm_bitfield gemm_flags, libxsmm_bitfield prefetch_flags,
  libxsmm_spgemm_config spgemm_config, int nshards, const int* devices);
LIBXSMM_API libxsmm_hip_sharded_kernel* libxsmm_hip_fsspmdm_create_sharded(libxsmm_datatype datatype, libxsmm_blasint M, libxsmm_blasint N, libxsmm_blasint K, libxsmm_blasint lda,
  const void* alpha, const void* beta, const void* a_dense, int nshards, const int* devices);
/** number of (non-empty) shards; shard i's device, its range [begin, end) of the split axis (P columns, M-blocks, N columns) and its plain handle
 * (a libxsmm_gemmfunction; owned by the set) */
LIBXSMM_API int libxsmm_hip_sharded_count(const libxsmm_hip_sharded_kernel* set);
LIBXSMM_API int libxsmm_hip_sharded_range(const libxsmm_hip_sharded_kernel* set, int shard, int* device, size_t* begin, size_t* end);
LIBXSMM_API libxsmm_gemmfunction libxsmm_hip_sharded_handle(const libxsmm_hip_sharded_kernel* set, int shard);
LIBXSMM_API int libxsmm_hip_sharded_launch(libxsmm_hip_sharded_kernel* set, const libxsmm_gemm_param* shard_params, int gather_device, void* gather_dst, size_t gather_dst_pitch);
LIBXSMM_API void libxsmm_hip_sharded_destroy(libxsmm_hip_sharded_kernel* set);

/* Result gather onto one GPU without a collective library (one process per GPU on one node).  Every rank exports the device buffer that
 * holds its shard (libxsmm_hip_ipc_export: LIBXSMM_HIP_IPC_HANDLE_BYTES opaque bytes, to be handed to the root by whatever means the
 * application has -- MPI, a file, torch.distributed); the root then pulls all shards, each on its own stream: the sources sit behind
 * different xGMI links of the root, so the copies overlap (up to world - 1 links) where a ring all-gather is bound by one link per hop.
 *   handles     : world x LIBXSMM_HIP_IPC_HANDLE_BYTES, entry r = what rank r exported (entry self_rank is ignored)
 *   self_src    : the root's own shard (plain device pointer)
 *   src_offsets : byte offset of the shard behind each exported pointer (NULL: all 0);  dst_offsets / nbytes: placement and size in dst
 * Returns 0 on success; the copies are complete on return.  The exporting ranks must keep their buffers alive until then. */
#define LIBXSMM_HIP_IPC_HANDLE_BYTES 80
LIBXSMM_API int libxsmm_hip_ipc_export(const void* device_ptr, void* handle);
LIBXSMM_API int libxsmm_hip_gather_shards(void* dst, int world, int self_rank, const void* handles, const void* self_src,
  const size_t* src_offsets, const size_t* dst_offsets, const size_t* nbytes);

/* ---- input preparation (the reference keeps these in its samples) ----------------------------------------
 * libxsmm_hip_mtx_read: Matrix-Market coordinate file -> CSR (by_column = 0: ptr over rows, idx = columns) or CSC (by_column = 1), values as
 * F32 or F64, entries in any order, empty rows / columns allowed [ref: samples/xgemm_norm_packed/common_edge_proxy.h:29-320].
 * libxsmm_hip_bcsc_from_dense: dense K x N operand stored as the reference's BCSC driver stores it (B[n*K + k]) -> colptr / rowidx / block values
 * [blk][bn][bk], all-zero blocks dropped [ref: samples/xgemm_sparse/spmm_kernel.c:306-347].
 * Every output array comes from libxsmm_aligned_malloc (device-visible pinned memory when a device is present): pattern arrays can be passed to
 * libxsmm_create_packed_spgemm_* / the BCSC call and value arrays to a.primary / b.primary as they are; release them with libxsmm_free.
 * Return EXIT_SUCCESS or EXIT_FAILURE (unreadable file, inconsistent header, index out of range, block sizes that do not divide). */
LIBXSMM_API int libxsmm_hip_mtx_read(const char* path, int by_column, libxsmm_datatype value_type, unsigned int** ptr, unsigned int** idx, void** values,
  unsigned int* rows, unsigned int* cols, unsigned int* nnz);
LIBXSMM_API int libxsmm_hip_bcsc_from_dense(libxsmm_datatype type, const void* dense, int K, int N, int bk, int bn,
  unsigned int** colptr, unsigned int** rowidx, void** values, unsigned int* nnzb);

/** BCSC kernels take their block pattern with every call (b.secondary = colptr, b.tertiary = rowidx, b.quaternary -> block-column count
 * [ref: samples/xgemm_sparse/spmm_kernel.c:423-456]) and need it inverted (block id per (block column, k-block)).  A pattern in HOST memory -- the
 * reference's convention -- is recognised by content and its inverted image cached with the kernel (no allocation, no lock on a hit).  A pattern in
 * DEVICE memory cannot be compared without a host round trip: by default it is inverted by a small kernel in front of every call; this function
 * lets the caller promise that the two device arrays do not change until the binding is replaced (NULL, NULL unbinds), so the table is built once,
 * stream-ordered on the calling thread's stream, and calls that pass exactly these pointers launch the GEMM kernel alone.  Outside a graph capture the
 * two arrays are also read once (the call then waits for the stream): the number of blocks and the k-blocks in use let the launcher pick the kernels
 * that keep a small B in LDS, as a host-resident pattern does. */
LIBXSMM_API int libxsmm_hip_bcsc_bind_pattern(libxsmm_gemmfunction kernel, const unsigned int* colptr, const unsigned int* rowidx, unsigned long long n_block_columns);

/* ---- run-time specialisation of the fixed-pattern sparse kernels ---------------------
 * libxsmm_create_packed_spgemm_csr/_csc, libxsmm_create_spgemm_csr_areg and libxsmm_fsspmdm_create can compile a
 * kernel with the sparsity pattern unrolled into the instruction stream (hiprtc), as the reference's JIT does
 * [ref: src/generator_packed_spgemm_csr_asparse_avx_avx2_avx512.c:336-470].  mode 0: never (precompiled LDS-staged
 * kernels), 1: when one call is large enough to repay the compile time (default), 2: always.
 * LIBXSMM_HIP_JIT=0|1|2 presets it.  Applies to kernels created afterwards. */
LIBXSMM_API void libxsmm_hip_set_jit(int mode);
LIBXSMM_API int libxsmm_hip_get_jit(void);

/* ---- introspection used by the tests and the bench --------------------------------- */
/** Name of the device kernel a handle launches for single (batch==0) or batched calls. */
LIBXSMM_API const char* libxsmm_hip_kernel_name(const void* kernel, int batched);
/** Number of kernel launches issued by the calling thread since the last reset. */
LIBXSMM_API unsigned long long libxsmm_hip_launch_count(int reset);
/** Diagnostic: what the matrix pipe of THIS chip sustains under its power budget.  Every wave (one per SIMD on every CU, 16 accumulators) issues
 * `iterations` x 16 MFMAs back to back on REGISTER operands taken from `operands` (device memory, 64 KiB of bf16 or f32 values) -- no LDS, no memory
 * traffic -- on the calling thread's stream.  datatype BF16: v_mfma_f32_32x32x16_bf16, F32: v_mfma_f32_32x32x2_f32.  *flop receives the floating-point
 * operations of the launch; time it with events.  The rate depends on the operand VALUES (zeros: 99 % of the 2.5 PF bf16 figure at 2.36 GHz; the reference
 * drivers' value distribution: 73 % at 1.75 GHz, profiles/r03_bf16_macro_ablation.txt): the roof a GEMM on the same data cannot exceed. */
LIBXSMM_API int libxsmm_hip_probe_mfma(libxsmm_datatype datatype, const void* operands, int iterations, double* flop);
/** 1 if the library was built with the gfx950 code object and a device is present. */
LIBXSMM_API int libxsmm_hip_available(void);

#endif /* LIBXSMM_HIP_H */
