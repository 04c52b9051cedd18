/*
 * remap_hip.h -- C ABI of libremap_hip.so, the MI355X (gfx950) weight-
 * application engine behind pyremap's Remapper.remap_numpy()/ncremap().
 *
 * The reference (MPAS-Dev/pyremap v2.4.0) is pure Python and has no FFI
 * boundary of its own; the seam this library replaces is the arithmetic of
 *
 *   pyremap/remapper/remap_numpy.py:134-137   COO triplets -> scipy CSR
 *                                             -> remap_csr_from_coo()
 *   pyremap/remapper/remap_numpy.py:258-278   masked / unmasked SpMM,
 *                                             normalisation and masking
 *                                             -> remap_apply_f64()
 *   pyremap/remapper/remap_numpy.py:254-256,  permute/flatten and
 *                                   280-295   unflatten/unpermute: absorbed
 *                                             into the batch/row strides of
 *                                             remap_apply_args (no copies)
 *   pyremap/remapper/remap_numpy.py:201-204   `isnan(values).any()` picks the
 *                                             masked or the unmasked branch
 *                                             -> remap_scan_nan() + two calls
 *                                             gated on its flag
 *                                             (remap_apply_args.gate)
 *   (no counterpart in the reference)         which kernel schedule a mapping
 *                                             gets, and building it on the
 *                                             device -> remap_schedule_auto()
 *                                             (remap_groups_build() and
 *                                             remap_patches_build() are its
 *                                             two builders, also exported)
 *   pyremap/remapper/remap_numpy.py:72-139    `_load_mapping` as a whole and
 *                                   223-297   `_remap_numpy_array` as a whole
 *                                             behind one opaque handle whose
 *                                             device memory the library owns
 *                                             -> remap_plan_create() /
 *                                             remap_plan_apply() /
 *                                             remap_plan_destroy()
 *
 * Conventions: extern "C"; plain pointers and sizes only; every pointer
 * marked (device) is an address in the current HIP device's memory (e.g.
 * torch.Tensor.data_ptr()); all launches are asynchronous on the caller's
 * hipStream_t (passed as void*; NULL = the null stream); nothing is allocated,
 * freed or synchronised inside the apply calls, so they are graph-capturable
 * (only remap_plan_create / _destroy allocate and free device memory).
 * Return value: REMAP_OK (0) or a negative REMAP_ERR_*; the message of the
 * last failure on the calling thread is available from remap_last_error().
 *
 * The reference-side binding (ctypes) is in pyremap_amd/engine.py; the stub a
 * pyremap maintainer would add is shown in INTEGRATION.md.
 */
#ifndef REMAP_HIP_H
#define REMAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REMAP_ABI_VERSION 31

/* The library is built with -fvisibility=hidden: the entry points declared
 * here, and nothing else, are its dynamic symbols. */
#if defined(__GNUC__) || defined(__clang__)
#define REMAP_API __attribute__((visibility("default")))
#else
#define REMAP_API
#endif

enum {
    REMAP_OK = 0,
    REMAP_ERR_ARG = -1,         /* bad argument (NULL, negative size, ...)  */
    REMAP_ERR_UNSUPPORTED = -2, /* valid request this build cannot serve    */
    REMAP_ERR_HIP = -3,         /* a HIP runtime call or launch failed      */
    REMAP_ERR_WORKSPACE = -4    /* workspace too small                      */
};

/* element type of the source field X (the output is always float64, as in the
 * reference: S is float64 and scipy upcasts, remap_numpy.py:264-268) */
enum { REMAP_DTYPE_F64 = 0, REMAP_DTYPE_F32 = 1 };

/* what is computed after num = A.X */
enum {
    /* Y = A.X, nothing else (the bare `matrix.dot`, remap_numpy.py:268) */
    REMAP_MODE_RAW = 0,
    /* unmasked branch, remap_numpy.py:268-278: den = frac_b[row];
     * Y = den > 0 ? num / den : NaN.  NaNs in X propagate. */
    REMAP_MODE_FRACB = 1,
    /* masked branch, remap_numpy.py:262-266,277-278, with the mask taken
     * from NaN in X (as _remap_data_array builds it, :201-204):
     * num = A.(X, NaN->+0), den = A.(!isnan X); Y = den > threshold ?
     * num / den : NaN. */
    REMAP_MODE_MASKED = 2,
    /* largest area fraction (CDO's remaplaf), for fields whose values are
     * labels -- region ids, land-cover classes, 0/1/2 flags: no num at all,
     * every destination element takes the source value whose weights in its
     * row add up to the most.  (An added enumerator of ABI 31: no existing
     * caller changes, the version stays.)  For destination element (i, b, k)
     * the entries j of row i are walked in CSR order, which is ascending
     * source cell:
     *   x = (double) X[cell(col_j), b, k]
     *   a NaN x is skipped; +-inf are values like any other
     *   the entry's class is the first earlier counted value of the row with
     *   value == x (so -0.0 and +0.0 are one class, and the class keeps the
     *   bits of its first member); no such value: a new class, w_c = +0.0
     *   w_c = w_c + S_j;   valid = valid + S_j
     *   (valid starts at +0.0; every sum rounded, in CSR order)
     *   winner: the classes in order of first appearance; the first one sets
     *   best; a later one replaces it iff w_c > best
     *   (strict: the first seen wins a tie; a NaN sum never replaces)
     *   y = (a class exists && valid > threshold) ? the winner's value : NaN
     * Every NaN written is 0x7ff8000000000000; mask_out, where given, gets 1
     * where NaN was written and 0 elsewhere.  Nothing is multiplied or
     * divided: REMAP_FLAG_FMA, REMAP_FLAG_TREE and the mask hints have no
     * meaning and are ignored, and so are frac_b, tune, row_order and every
     * attached schedule (patch plan, row groups, share lists, strips): the
     * mode picks its own launch (csrc/apply_laf.h).  gate / gate_value are
     * honoured, rows outside [row_begin, row_end) are not written, x_dtype
     * F64 and F32 are served (float32 widens exactly), x_src_fold and every
     * stride are addressed as in the other modes.  Signed weights
     * (conserve2nd, patch, a file) are legal: the sums are what they are. */
    REMAP_MODE_LAF = 3,
    /* (4 to 7 are not assigned: "unknown mode") */
    /* Sub-grid statistics (CDO's remapmin, remapmax, remapvar, remapmedian):
     * what the spread of the source values under a destination cell is --
     * the roughness of a topography, the shallowest and deepest depth, a
     * median that outliers do not pull.  (Added enumerators of ABI 31: no
     * existing caller changes, the version stays.)
     * For destination element (i, b, k) the entries j of row i are walked in
     * CSR order:
     *   x_j = (double) X[cell(col_j), b, k]
     *   an entry counts iff x_j is no NaN; +-inf are values like any other
     *   valid starts at +0.0; for every counted entry, in CSR order,
     *   valid = valid + S_j, each sum rounded
     *   ok = (some entry counts) && valid > threshold; where !ok, y = NaN
     * MIN / MAX:
     *   the first counted x sets m; after it, if (x < m) m = x  (MAX: >)
     *   strict, so the first seen wins a tie and -0.0 against +0.0 is
     *   decided by CSR order (remap_limit_rows has the same rule)
     *   weights enter only through valid; y = m
     * VAR (weighted population variance, in two walks):
     *   walk 1: num starts at +0.0; for counted entries
     *   num = num + (S_j * x_j), the product rounded and the sum rounded;
     *   mean = num / valid
     *   walk 2: m2 starts at +0.0; for counted entries d = x_j - mean;
     *   m2 = m2 + (S_j * (d * d)), every operation rounded, no FMA
     *   contraction
     *   y = m2 / valid; a NaN result is written as the canonical NaN (an inf
     *   among the values gives inf - inf)
     * MEDIAN (lower weighted median, needs no table):
     *   half = 0.5 * valid
     *   for a counted entry j, below_j starts at +0.0 and adds S_q, in CSR
     *   order, over the counted q of the row with x_q <= x_j (j itself
     *   included)
     *   j qualifies iff below_j >= half
     *   y is the least x_j among the qualifying entries (strict <: the first
     *   seen wins a tie); none qualifies: y = NaN
     * Every NaN written is 0x7ff8000000000000; mask_out, where given, gets 1
     * where NaN was written and 0 elsewhere.  No division but num / valid
     * and m2 / valid, no transcendental: the standard deviation is the
     * caller's square root of VAR.  As in REMAP_MODE_LAF, flags, tune,
     * frac_b, row_order and every attached schedule are ignored and the
     * modes pick their own launch (csrc/apply_rowstat.h); gate / gate_value
     * are honoured, rows outside [row_begin, row_end) are not written,
     * x_dtype F64 and F32 are served (float32 widens exactly), x_src_fold
     * and every stride are addressed as in the other modes.  Signed weights
     * (conserve2nd, patch) are legal and give what the definition gives;
     * with non-negative weights MEDIAN is the usual weighted median. */
    REMAP_MODE_MIN = 8,
    REMAP_MODE_MAX = 9,
    REMAP_MODE_VAR = 10,
    REMAP_MODE_MEDIAN = 11,
    /* (12 is not assigned: "unknown mode") */
    /* Sub-grid composition: what share of a destination cell every class or
     * value range takes -- percent cover per land-cover type, elevation and
     * depth bands (a histogram of a continuous field whose values the caller
     * turned into bin indices), fractional region masks.  REMAP_MODE_LAF is
     * the argmax of exactly these sums.  (An added enumerator of ABI 31: no
     * existing caller changes, the version stays.)
     * The arguments are read in their own way:
     *   X holds class indices as numbers (x_dtype F64 or F32) and is ONE
     *   batch: x_batch_stride must be 0 (REMAP_ERR_ARG otherwise);
     *   n_batch is the number of classes C, 1 <= C <= 256 (REMAP_ERR_ARG
     *   beyond: 8-bit rasters, and a result of (C, n_b, k_inner));
     *   the batches of Y, and of mask_out where given, are the classes:
     *   Y[c * y_batch_stride + i * y_row_stride + k].
     * For destination element (i, k) the entries j of row i are walked in
     * CSR order:
     *   x = (double) X[cell(col_j), k]
     *   the entry counts iff x is no NaN; then valid = valid + S_j
     *   a counted entry belongs to class c iff x == (double) c for an integer c
     *   in [0, C); -0.0 is class 0; a non-integer, +-inf or a value outside the
     *   range counts in valid alone
     *   w_c = w_c + S_j for the entry's class and for no other
     *   valid and every w_c start at +0.0; every sum rounded, in CSR order
     *   y_c = valid > threshold ? w_c / valid : NaN, for every c: one division
     *   a NaN quotient is written as the canonical NaN 0x7ff8000000000000
     * mask_out, where given, gets 1 where NaN was written and 0 elsewhere.
     * With every value a class the fractions of an element add up to 1 within
     * rounding; a value that is no class lowers the sum.  flags, tune, frac_b,
     * row_order and every attached schedule are ignored and the mode picks its
     * own launch (csrc/apply_classfrac.h); x_src_fold, x_outer_stride,
     * row_begin / row_end and gate / gate_value work as in REMAP_MODE_LAF.
     * Through remap_plan_apply the mode gives REMAP_ERR_UNSUPPORTED on a plan
     * that keeps long rows apart, as LAF does.  Signed weights (conserve2nd,
     * patch) are legal and give what the definition gives. */
    REMAP_MODE_CLASSFRAC = 13,
    /* (14 and 15 are not assigned: "unknown mode") */
    /* The cotangent of the division: the first step of the adjoint apply,
     * which carries a cotangent G of a forward result y back to the field X
     * (gX = dL/dX for G = dL/dy).  (Added enumerators of ABI 31: no existing
     * caller changes, the version stays.)  S is the plan's CSR, (n_b, n_a); X
     * the forward's field; G has the shape and layout of the forward's
     * result; gX has the shape of X.
     * 1. Cotangent of the division, T by destination element (i, b, k) --
     *    these two modes; a masked element is a selection, not a product:
     *   forward REMAP_MODE_RAW: T = G (no launch)
     *   REMAP_MODE_COTAN_FRACB (forward REMAP_MODE_FRACB):
     *   T = frac_b_i > 0 ? G / frac_b_i : +0.0
     *   REMAP_MODE_COTAN_MASKED (forward REMAP_MODE_MASKED):
     *   den starts at +0.0; for the entries j of row i, in CSR order,
     *   den = den + S_j iff X[cell(col_j), b, k] is no NaN, each sum rounded
     *   (the forward's own den)
     *   T = den > threshold ? G / den : +0.0, one IEEE division
     *   where the forward wrote NaN, G is not looked at, even if it is NaN
     * 2. Transposed sum: REMAP_MODE_RAW applied with the canonical CSR of S^T
     *    (within a source cell its entries in ascending destination row),
     *    flags 0, exactly:
     *   acc starts at +0.0; acc = acc + (S_ij * T_i), the product rounded, then
     *   the sum; no FMA; an empty column gives +0.0
     * 3. Missing sources (MASKED forward only):
     *   gX = +0.0 where X is NaN
     * The arguments are read in their own way:
     *   A is S;
     *   Y holds G on entry and T on exit: every element in rows [row_begin,
     *   row_end) is read once and then written once, through the y_* strides;
     *   X is the forward's field, read for NaN only: x_dtype F64 and F32 are
     *   served, the x_* strides, x_src_fold and x_outer_stride are those of
     *   the forward launch; REMAP_MODE_COTAN_FRACB does not read X and it may
     *   be NULL (x_dtype and the x_* strides are still checked);
     *   frac_b is used by REMAP_MODE_COTAN_FRACB only (REMAP_ERR_ARG if
     *   NULL), threshold by REMAP_MODE_COTAN_MASKED only;
     *   mask_out must be NULL (REMAP_ERR_ARG);
     *   gate / gate_value are honoured: rows outside the range and a closed
     *   gate leave Y untouched;
     *   flags, tune, row_order and every attached schedule are ignored and the
     *   modes pick their own launch (csrc/apply_cotangent.h).
     * Through remap_plan_apply the modes give REMAP_ERR_UNSUPPORTED on a plan
     * that keeps long rows apart, as REMAP_MODE_LAF does.  Signed weights and
     * a negative threshold are legal and give what the definition gives. */
    REMAP_MODE_COTAN_FRACB = 16,
    REMAP_MODE_COTAN_MASKED = 17,
    /* (18 and 19 are not assigned: "unknown mode") */
    /* One pass of a creeping fill: missing cells of a field take values from
     * their valid neighbours on the SAME grid (compass' extrap_woa, CDO's
     * fillmiss / setmisstonn, ESMF's --extrap_method creep); repeated by the
     * caller between two buffers until nothing fillable is left, one more
     * ring of cells per pass.  (Added enumerators of ABI 31: no existing
     * caller changes, the version stays.)
     * The arguments are read in their own way:
     *   A is the neighbour matrix of the grid: square (REMAP_ERR_ARG
     *   otherwise), row i holding the neighbours of cell i and their weights,
     *   no diagonal entry needed;
     *   X is a field on that grid, Y the filled field; Y must not be X: equal
     *   pointers give REMAP_ERR_ARG.
     * For element (i, b, k), with x_i = (double) X[cell(i), b, k]:
     *   x_i is no NaN: y = x_i (a copy: float32 widens exactly), mask 0
     *   x_i is NaN: the entries j of row i are walked in CSR order (ascending col)
     *     x_j = (double) X[cell(col_j), b, k]
     *     an entry counts iff x_j is no NaN; +-inf are values like any other
     *   FILL_BEST: the first counted entry sets best = S_j, v = x_j; a later one
     *     replaces both iff S_j > best (strict: the lowest col wins a tie, a NaN
     *     S_j never replaces)
     *     y = some entry counts ? v : NaN
     *   FILL_MEAN: num and den start at +0.0; for every counted entry, in CSR order,
     *     num = num + (S_j * x_j), den = den + S_j, the product rounded, then each
     *     sum; no FMA contraction
     *     y = den > threshold ? num / den : NaN, one IEEE division
     * Every NaN written is 0x7ff8000000000000; mask_out, where given, gets 1 where
     * NaN was written and 0 elsewhere.  Only X is read: no value written by this
     * launch is looked at.
     * The arguments are otherwise read as in REMAP_MODE_LAF: flags, tune,
     * frac_b, row_order and every attached schedule are ignored and the
     * modes pick their own launch (csrc/apply_fill.h); gate / gate_value are
     * honoured, rows outside [row_begin, row_end) are not written, x_dtype
     * F64 and F32 are served, every stride, x_src_fold and x_outer_stride
     * address cells as in the other modes, for the element's own cell too.
     * threshold is used by FILL_MEAN only.  Through remap_plan_apply the
     * modes give REMAP_ERR_UNSUPPORTED on a plan that keeps long rows apart.
     * With non-negative weights FILL_MEAN at a missing element is byte for
     * byte REMAP_MODE_MASKED of the same matrix, field and threshold: the
     * whole pass is where(isnan(X), masked apply, X). */
    REMAP_MODE_FILL_BEST = 20,
    REMAP_MODE_FILL_MEAN = 21
};

enum {
    /* accumulate with fused multiply-add.  Default (flag clear) is a separate
     * multiply and add in CSR order, which is bit-identical to scipy's
     * csr_matvecs; FMA is within 1 ulp per term of it, not identical. */
    REMAP_FLAG_FMA = 1u << 0,
    /* bit 1 is unused (it once asked for write-back instead of non-temporal
     * stores of Y; non-temporal measured faster on every configuration) */
    /* `tune` is a preference, not a demand: if the requested kernel family
     * cannot serve this call (K <= 32, odd strides, a partial row range, a
     * missing schedule ...) choose automatically instead of failing */
    REMAP_FLAG_TUNE_HINT = 1u << 2,
    /* calls served by kernel family 3 (K <= 32, opt-in) may add a row's products
     * by lane-private partial sums and a butterfly across lanes instead of
     * one after the other in CSR order: a different association, within
     * 1e-13 relative of the default -- for callers that do not need the
     * bits.  Ignored by the other kernel families. */
    REMAP_FLAG_TREE = 1u << 3,
    /* REMAP_MODE_MASKED, a HINT: the caller expects a source cell to be
     * valid in all of the call's columns or missing in all of them (land, an
     * ice shelf, no NaN at all in most of the field) rather than column by
     * column (a 3-D field cut by bathymetry).  On mappings scheduled as
     * 8-row groups (entry-rich: 2nd-order conservative) the normaliser
     * `A . [not isnan X]` (remap_numpy.py:265) is then kept per ROW, with
     * two K tiles per wave as in the frac_b mode; groups where the
     * expectation fails are redone with per-lane normalisers inside the
     * same launch.  Same bits with or without the flag, whatever the data;
     * only the speed differs (config 5: 27.4 -> 22.0 ms with whole cells
     * missing, 26.7 -> 35.3 with the flag set on a bathymetry mask).
     * remap_scan_nan_kinds() tells the two apart on the device.  Ignored
     * elsewhere. */
    REMAP_FLAG_CELL_MASKS = 1u << 4,
    /* REMAP_MODE_MASKED on a field of several batches, a HINT (ABI 25): the
     * mask is expected to be the same in every batch -- a (Time, nCells,
     * nVertLevels) ocean variable is missing below the sea floor at every
     * time.  The reference sums the normaliser `A . [not isnan X]` for every
     * column of every time slice (remap_numpy.py:265); on mappings scheduled
     * as 8-row groups a wave then takes four time slices of a level per lane
     * and keeps ONE normaliser for them (csrc/spmm_grouptime.h).  Groups
     * where the expectation fails are redone with per-element normalisers
     * inside the same launch: same bits with or without the flag, whatever
     * the data.  Needs n_batch >= 3; ignored elsewhere.  The device-side
     * scan remap_scan_nan_layout() tells whether it holds. */
    REMAP_FLAG_BATCH_MASKS = 1u << 5
};

/* CSR weight matrix of shape (n_rows, n_cols) = (n_b, n_a), or a row shard of
 * it (rows [r0, r1) of the full matrix with rowptr rebased to 0). */
typedef struct remap_csr {
    int64_t n_rows;
    int64_t n_cols;
    int64_t nnz;
    const int64_t *rowptr; /* (device) n_rows + 1                            */
    const int32_t *col;    /* (device) nnz, ascending within a row, 0-based  */
    const double *val;     /* (device) nnz                                   */
    int64_t max_row_nnz;   /* entries of the longest row, 0 = unknown (lets
                              the library pick kernels specialised for short
                              rows; a wrong value only costs speed if too
                              large, but MUST NOT be smaller than the truth) */
    int64_t csr_pad;       /* readable (don't-care) entries allocated behind
                              col[nnz-1] and val[nnz-1]; >= 8 enables the
                              kernels that fetch a row's entries 8 at a time
                              through the scalar cache                       */
} remap_csr;

/*
 * Optional strip schedule of kernel family 8 (remap_apply_args.strips; built
 * by the host layer: pyremap_amd.engine.RemapPlan.build_strips).  For
 * entry-rich mappings onto a 2-D destination grid (2nd-order conservative
 * stencils: 12-30 entries per row): the grid is cut into strips of
 * `strip_rows` grid rows, a strip into segments, a segment is walked in steps
 * of `step_cols` grid columns.  Unit u = one (strip, segment); its steps are
 * g = u * steps_per_unit + t, t < unit_steps[u].  A workgroup owns one (unit,
 * 64-column K-chunk): the 512-byte pieces of the source rows a step needs
 * ARRIVE in an LDS ring of `ring_slots` slots, `depth` steps ahead, and stay
 * while consecutive steps use them; the rows of a step are dealt to 8
 * compute waves, `rows_per_wave` each.  Every row still adds its entries in
 * ascending column order: results are unchanged.
 * The schedule is TRUSTED: the library checks the scalar fields only.  At
 * most 64 arrival pairs per step, arrival slots below ring_slots / 2, record
 * offsets and meta blocks inside meta_slot_bytes are the builder's to keep
 * (pyremap_amd/strips.py does, tests/test_strips_cpu.py replays it); a
 * schedule that breaks them makes the LDS-DMA write outside the ring.  Build
 * it with pyremap_amd.strips.build_strips or leave `strips` NULL.
 */
typedef struct remap_strips {
    int64_t n_units;
    int32_t steps_per_unit;
    int32_t rows_per_wave;      /* ceil(strip_rows * step_cols / waves)      */
    int32_t ring_slots;         /* piece slots, even: ring_slots * 512 bytes */
    int32_t depth;              /* steps an arrival is issued ahead: 1 .. 6
                                   (= loader waves per workgroup)            */
    int32_t meta_slot_bytes;    /* largest meta block, rounded up to 1 KiB;
                                   (depth + 1) such slots follow the piece
                                   slots and 1 KiB holding a slot of zeros   */
    int32_t waves;              /* compute waves per workgroup the rows of a
                                   step are dealt to; waves + depth <= 16    */
    const int32_t *unit_steps;  /* (device) n_units                          */
    /* arrival pairs of step g: i in [arr_ptr[g], arr_ptr[g + 1]); pair i
     * brings the pieces of source rows arr_src[2 i] and arr_src[2 i + 1]
     * (-1: none) into slots 2 arr_slot[i] and 2 arr_slot[i] + 1. */
    const int32_t *arr_ptr;     /* (device) n_units * steps_per_unit + 1     */
    const int32_t *arr_src;     /* (device) 2 per pair                       */
    const int32_t *arr_slot;    /* (device) 1 per pair                       */
    /* meta block of step g: 16-byte units [meta_ptr[g], meta_ptr[g + 1]) of
     * `meta`.  First waves * rows_per_wave row headers of 32 bytes, work
     * slot wave * rows_per_wave + i: {int32 row id (-1: none), int32 first
     * record, int32 records (a multiple of 4), 0; double frac_b, 0}; then
     * the step's records, 16 bytes each, a row's entries in ascending column
     * order followed by its pads: {int32 byte offset of the source row's
     * piece in LDS (slot * 512; pads: ring_slots * 512, the slot of zeros),
     * 0; double weight (pads: +0.0)}. */
    const int64_t *meta_ptr;    /* (device) n_units * steps_per_unit + 1     */
    const void *meta;           /* (device) 16-byte aligned (+ 1 KiB readable) */
} remap_strips;

/*
 * Two levels.  The PUBLIC, frozen face for a binder is
 * the opaque plan handle further down -- remap_plan_create / _apply /
 * _destroy with the 15-field remap_field -- which hides every schedule
 * internal.  remap_apply_args below is the ADVANCED level: the non-allocating
 * entry points a host layer with its own allocator composes (this package's
 * Python layer does); its schedule fields mirror remap_schedule one to one
 * and are filled by remap_schedule_auto, not by hand.
 *
 * One application of the weights to a batch of fields.
 *
 * The flattened (n_a, K) matrix of the reference (remap_numpy.py:254-256) is
 * addressed in place: K = n_batch * k_inner and flat column kf = b * k_inner
 * + k lives at X[b * x_batch_stride + a * x_row_stride + k] (strides in
 * elements, the k index contiguous).  A field laid out (n_a, K) has
 * n_batch = 1; an MPAS field (Time, nCells, nVertLevels) has n_batch = Time,
 * k_inner = nVertLevels, x_row_stride = nVertLevels, x_batch_stride =
 * nCells * nVertLevels.  Y is addressed the same way with its own strides, so
 * the output lands directly in the reference's final axis order
 * (remap_numpy.py:280-295).
 */
typedef struct remap_apply_args {
    remap_csr A;
    int64_t row_begin;      /* rows [row_begin, row_end) of A are computed;  */
    int64_t row_end;        /* Y / frac_b / mask_out are indexed by row      */
    const void *X;          /* (device) source field                         */
    int32_t x_dtype;        /* REMAP_DTYPE_*                                 */
    int32_t mode;           /* REMAP_MODE_*                                  */
    int64_t x_row_stride;
    int64_t x_batch_stride;
    double *Y;              /* (device) destination field, float64           */
    int64_t y_row_stride;
    int64_t y_batch_stride;
    int64_t n_batch;
    int64_t k_inner;
    const double *frac_b;   /* (device) n_rows; REMAP_MODE_FRACB only        */
    double threshold;       /* REMAP_MODE_MASKED, _LAF, _MIN .. _MEDIAN      */
    uint8_t *mask_out;      /* (device) optional, addressed like Y; 1 where
                               the reference's result is masked (~ok)        */
    const int32_t *row_order; /* (device) optional processing order: entry s
                               (row_begin <= s < row_end) names the row that
                               work slot s computes; must be a permutation of
                               [row_begin, row_end).  Scheduling only -- the
                               results do not depend on it.  Used to walk a
                               2-D destination grid in tiles so neighbouring
                               rows (which share source rows) run together
                               and re-touches hit the XCD's L2.             */
    /* Optional LDS-staging schedule ("patch plan", all NULL/0 = absent).
     * Work slots [row_begin + j*patch_rows, +patch_rows) form patch j (with
     * row_order, a 2-D tile of the destination grid).
     *   patch_ucol   per patch, the DISTINCT source rows its entries
     *                reference (ascending); patch_ptr[j] .. patch_ptr[j+1]
     *                delimits patch j's list;
     *   patch_rowptr / patch_lidx / patch_val: the weights again, laid out
     *                in SLOT order (patch-major CSR): slot s owns entries
     *                patch_rowptr[s - row_begin] .. patch_rowptr[s - row_begin
     *                + 1], in the row's CSR order; patch_lidx[e] is the
     *                position of that entry's column in its patch's list and
     *                patch_val[e] its weight.
     * The kernel fetches each distinct source row ONCE per patch into LDS
     * (together with the patch's entries) and serves the patch's
     * ~nnz/n_a-fold re-touches from there.  Results are unaffected (same
     * per-row summation order).                                          */
    const int32_t *patch_ptr;    /* (device) n_patches + 1                  */
    const int32_t *patch_ucol;   /* (device) patch_ptr[n_patches]           */
    const int32_t *patch_rowptr; /* (device) row_end - row_begin + 1        */
    const int32_t *patch_lidx;   /* (device) nnz                            */
    const double *patch_val;     /* (device) nnz                            */
    int32_t patch_rows;          /* work slots per patch                    */
    int32_t patch_umax;          /* longest per-patch list (sizes the LDS)  */
    int32_t patch_emax;          /* most entries in one patch               */
    int32_t patch_row_bytes;     /* staged bytes per source row and K-chunk:
                                    1024 (128 columns) or 512 (64 columns)   */
    int64_t n_patches;
    /* Optional row-group schedule (all NULL/0 = absent): with G =
     * group_rows (8 or 4), work slots [row_begin + G g, + G) form group g
     * (with row_order: a 2 x 4 or 2 x 2 tile of the destination grid).
     * group_col lists, per group, the sorted UNION of its rows' columns;
     * bit m of group_mask[u] says whether the group's m-th row owns union
     * entry u; group_w holds the weights of exactly those present (entry,
     * member) pairs, in (entry, member) order -- nnz doubles in all;
     * group_meta[2 g] / [2 g + 1] index group g's first union entry / first
     * weight (entry n_groups closes the lists).  group_rid / group_frac give
     * the row id / frac_b of every work slot, padded to whole groups (the
     * pad names any valid row).  A wave then loads every distinct source
     * row of G neighbouring destination rows ONCE and feeds up to G
     * accumulators from it; each row still adds its entries in ascending
     * column order, so results are unchanged.                              */
    const int64_t *group_meta;  /* (device) 2 * (n_groups + 1)              */
    const int32_t *group_col;   /* (device) union entries (+ 32 readable)   */
    const double *group_w;      /* (device) present weights (+ 128 readable) */
    const int32_t *group_mask;  /* (device) union entries (+ 32)            */
    const int32_t *group_rid;   /* (device) n_groups * group_rows           */
    const double *group_frac;   /* (device) n_groups * group_rows           */
    int64_t n_groups;
    int32_t group_rows;         /* G: 8 or 4 (16: float64, even strides)    */
    int32_t group_reserved;     /* must be 0                                */
    /* Optional device-side switch (NULL = always run): the launch does its
     * work only if the int32 at `gate` equals `gate_value` when the kernel
     * starts, and is a no-op otherwise.  With remap_scan_nan() this moves
     * the reference's `isnan(values).any()` decision (remap_numpy.py:201-204:
     * masked branch iff the field holds a NaN) onto the device: scan into a
     * flag, then enqueue the MASKED call gated on 1 and the FRACB call gated
     * on 0 -- no host synchronisation in between.                           */
    const int32_t *gate;    /* (device) optional                             */
    int32_t gate_value;
    uint32_t flags;         /* REMAP_FLAG_*                                  */
    /* launch tuning, 0 = choose automatically:
     * tune[0] kernel family   1 = wave per row (lanes across K),
     *                         2 = lane per (row, k) (small K),
     *                         3 = a sub-group of lanes per row, lanes across
     *                             the row's entries (K <= 32, opt-in: it
     *                             measured slower than 2; tune[1] = lanes
     *                             per row, 8 or 4),
     *                         5 = LDS-staged patches (needs a patch plan),
     *                         10 = G rows per wave over the union of their
     *                              columns (needs the row-group schedule),
     *                         6 = 1 with row metadata through the scalar
     *                             cache (needs csr_pad >= 8; the default)
     *                         4 = lanes across destination rows, TT fields
     *                             per lane (short contiguous runs in
     *                             several batches: (Time, nCells)),
     *                         7 = 4 with the distinct source cells of a
     *                             patch staged in LDS (needs a patch plan)
     *                         8 = an LDS ring sliding along strips of the
     *                             destination grid (needs `strips`)
     *                         9 = one wave per (row, few columns), the
     *                             row's entries read lanes-across-entries
     *                             and summed in order from LDS: for a CSR of
     *                             LONG rows (hundreds of entries) and few
     *                             fields.  `A` then holds those rows only:
     *                             its row r is work slot r and row_order[r],
     *                             if given, names the row of Y / frac_b /
     *                             mask_out it writes; needs A.max_row_nnz;
     *                             tune[1] = columns per wave (1 ... 16)
     *                         11 = one wave per LONG row x 64 columns, the
     *                             distinct source cells of a patch of R <=
     *                             16 consecutive long rows sliding through
     *                             LDS in windows of 8 R cells (many fields;
     *                             `A` and row_order as for 9).  Needs a
     *                             patch plan (remap_patches_build, tile 1 x
     *                             R, no patch_ell_base) whose patch_lidx do
     *                             not decrease inside a row -- true when the
     *                             rows of A are sorted by column
     * tune[1] doubles per lane per tile (1 or 2); family 10: waves per
     *         workgroup (1, 2; else 4); family 2: entries of a row fetched
     *         together (1, 4 or 8); family 5: threads per workgroup on
     *         64-column chunks (512 or 1024; 0: by the length of the work
     *         list)
     * tune[2] K tiles per wave (1, 2 or 4)
     * tune[3] consecutive rows per wave
     * tune[4] block -> work map: 1 = as dispatched, 2 = XCD-contiguous;
     *         family 10 also 3 = XCD-contiguous with the K-chunks of a row
     *         block side by side in the work list (the schedule of a group
     *         is fetched once per XCD: what remap_schedule_auto picks for
     *         entry-rich mappings)
     * tune[5] family 10: union entries in flight per wave (8; or 4, 16);
     *         26 / 28: the rolling form with 6 / 8 in flight (float64, even
     *         strides; spmm_grouproll.h: measured, not chosen); 9: keep the
     *         per-lane masked form under REMAP_FLAG_CELL_MASKS; 8 (the
     *         default count, said aloud): keep the 8-row groups under
     *         REMAP_FLAG_CELL_MASKS on a plan with share_* lists; 32: the
     *         shared form (share_* below: the frac_b and raw modes;
     *         tune[2] = K tiles per wave, 1 or 2)
     * tune[6..7] reserved, must be 0 (a -DREMAP_DIAG build of the library,
     *         tools/build_diag.py, reads bottleneck-analysis switches from
     *         them; this build rejects them) */
    int32_t tune[8];
    /* Two source axes that are NOT adjacent in memory -- a field (lat, M,
     * lon[, T]) remapped over (lat, lon): source cell a = y * x_src_fold + x
     * lives at y * x_outer_stride + x * x_row_stride (+ the column's offset
     * b * x_batch_stride + k, where the dims BETWEEN the two axes are the
     * batches: n_batch = M, x_batch_stride = their stride, k_inner = T).
     * x_src_fold = 0 (the default): one stride, a * x_row_stride.  Served in
     * place by the lanes-across-rows kernels (families 4 and 7); the
     * reference takes a transpose copy (remap_numpy.py:254-256). */
    int64_t x_src_fold;
    int64_t x_outer_stride;
    /* Family 7 only, optional (NULL: the patch plan's entries lie row after
     * row, patch_rowptr addressing them).  Not NULL: they lie COLUMN-MAJOR
     * inside every patch -- entry j of the patch's slot r at
     * patch_val / patch_lidx [patch_ell_base[patch] + j * patch_rows + r];
     * patch_rowptr then only gives the slots' entry counts -- so that the 64
     * lanes of a wave, one slot each, read their j-th entries with ONE
     * coalesced load.  For patches of LONG rows: the pole caps of a global
     * bilinear map as ESMF makes it, 362-1 442 entries per row, where a
     * lane reading its own row's entries one by one pays a line fetch per
     * lane and entry (engine.RemapPlan._split_long_rows). */
    const int64_t *patch_ell_base;
    /* Optional strip schedule (HOST pointer to a struct of device pointers;
     * NULL = absent), kernel family 8: the whole row range, float64 X, one
     * batch (n_batch == 1) of an even number of contiguous columns. */
    const remap_strips *strips;
    /* Optional SHARED union lists on top of an 8-row group schedule (all
     * NULL/0 = absent; ABI 25): share_waves (2 or 4) consecutive groups -- a
     * 4 x 4 or 4 x 8 tile of the destination grid when the groups were built
     * with super_tile = 4 or 8 -- form a SUPERGROUP served by one workgroup
     * of share_waves waves.  share_col lists, per supergroup, the sorted
     * union of the source rows its 8 * share_waves rows reference; bit
     * 8 w + m of share_mask[u] says whether member m of the supergroup's
     * w-th group owns union entry u; share_meta[2 s] is supergroup s's first
     * union entry (entry n_super closes the lists; the odd slots are not
     * read).  The weights are group_w of the 8-row schedule: its
     * (group, entry, member) order is every wave's own contiguous stream.
     * The workgroup sends each distinct source row of the supergroup ONCE
     * from global memory into an LDS ring (LDS-DMA) and every wave adds the
     * entries its own rows own from there (csrc/spmm_sharering.h); a row
     * still adds its entries in ascending column order, so results are
     * unchanged.  Used by family 10 on float64 fields with even strides:
     * with tune[5] = 32 in the frac_b and raw modes on at least 104
     * columns (one K tile per wave up to 128, two beyond) and on 34 ... 64
     * columns (a lane per column: csrc/spmm_narrowshare.h), with
     * REMAP_FLAG_BATCH_MASKS (csrc/spmm_timeshare.h) or, on
     * more than 128 columns, REMAP_FLAG_CELL_MASKS (csrc/spmm_cellshare.h)
     * in the masked mode (share_waves = 4: the shape the kernels are built
     * in; remap_share_build also makes the lists of 2 groups).             */
    const int64_t *share_meta;  /* (device) 2 * (n_super + 1)               */
    const int32_t *share_col;   /* (device) union entries (+ 256 readable)  */
    const int32_t *share_mask;  /* (device) union entries (+ 256 readable)  */
    int32_t share_waves;        /* 2 or 4                                   */
    int32_t share_reserved;     /* must be 0                                */
} remap_apply_args;

/* ABI / build information */
REMAP_API int remap_abi_version(void);
REMAP_API const char *remap_arch(void);       /* "gfx950" */
REMAP_API const char *remap_last_error(void); /* thread-local, never NULL */

/* Number of visible HIP devices, or a negative REMAP_ERR_HIP. */
REMAP_API int remap_device_count(void);

/*
 * Apply the weights (asynchronous on `stream`).  Replaces
 * remap_numpy.py:258-278 (and, through the strides, :254-256 and :280-295).
 */
REMAP_API int remap_apply_f64(const remap_apply_args *args, void *stream);

/*
 * COO -> CSR on the device: scipy's `csr_matrix((S, (row, col)))` of
 * remap_numpy.py:134-137.  Stable sort by (row, col), duplicates summed in
 * input order, explicit zeros kept.  `index_base` is subtracted from row and
 * col (1 for a SCRIP/ESMF mapping file).
 *
 *   rowptr_out (device) n_rows + 1;  col_out / val_out (device) nnz entries
 *   (only the first *nnz_out are meaningful);  nnz_out (device) one int64;
 *   bad_out (device) one int64: number of triplets whose row or col is out
 *   of range (the caller must treat non-zero as an error).
 *
 * All outputs are written asynchronously on `stream`.  Query the workspace
 * size first; the workspace is plain device memory owned by the caller.
 */
REMAP_API int remap_csr_from_coo_workspace(int64_t nnz, int64_t n_rows,
                                 size_t *bytes_out);
REMAP_API int remap_csr_from_coo(int64_t n_rows, int64_t n_cols, int64_t nnz,
                       const int32_t *row, const int32_t *col,
                       const double *S, int32_t index_base,
                       int64_t *rowptr_out, int32_t *col_out,
                       double *val_out, int64_t *nnz_out, int64_t *bad_out,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Build the row-group schedule of kernel family 10 (remap_apply_args.group_*)
 * for the rows of A on the device -- what a binder needs to reach the
 * kernels that carry the headline numbers without any host-side logic of its
 * own.  Asynchronous on `stream`; nothing is allocated.
 *
 *   A            the CSR whose rows are scheduled (a row shard: its rows,
 *                rowptr rebased to 0); canonical (remap_csr_from_coo's form)
 *   frac_b       (device) A.n_rows
 *   group_rows   G: 8, or 4
 *   grid_dims    (HOST) NULL: groups are G consecutive rows; else {my, mx},
 *                the C-order dims of the WHOLE destination grid: groups are
 *                2 x G/2 tiles of it, walked row-major inside super_tile x
 *                super_tile blocks (super_tile <= 0: over the whole grid)
 *   row_offset   index of A's first row in the whole grid (0 unless a shard)
 *   share_waves  0, or (ABI 25, group_rows = 8) 2 / 4: the group tiles are
 *                walked inside 4 x 4 / 4 x 8 tiles -- 2 / 4 consecutive
 *                groups, the supergroups of remap_share_build -- and those
 *                row-major inside the supertiles (a multiple of the tile)
 *   row_order_out (device, A.n_rows, may be NULL when grid_dims is NULL) the
 *                processing order the schedule assumes: pass it as
 *                remap_apply_args.row_order together with the schedule
 *   group_meta   (device) 2 * (n_groups + 1)     n_groups = ceil(n_rows / G)
 *   group_col, group_mask  (device) A.nnz + 32 each (union entries <= nnz)
 *   group_w      (device) A.nnz + 128
 *   group_rid, group_frac  (device) n_groups * G
 *   n_union_out  (device) one int64: union entries actually used
 */
REMAP_API
int remap_groups_workspace(int64_t n_rows, int64_t nnz, size_t *bytes_out);
REMAP_API int remap_groups_build(const remap_csr *A, const double *frac_b,
                       int32_t group_rows, const int64_t *grid_dims,
                       int64_t row_offset, int32_t super_tile,
                       int32_t share_waves,
                       int32_t *row_order_out, int64_t *group_meta,
                       int32_t *group_col, int32_t *group_mask,
                       double *group_w, int32_t *group_rid,
                       double *group_frac, int64_t *n_union_out,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Build the SHARED union lists of the shared form of family 10
 * (remap_apply_args.share_*; csrc/spmm_sharering.h) on top of an 8-row
 * group schedule remap_groups_build has made for the same rows: supergroup s
 * = work slots [8 * share_waves * s, + 8 * share_waves) of that schedule
 * (build it with the same share_waves, so that a supergroup is a 4 x 4 /
 * 4 x 8 tile of the destination grid).  Asynchronous
 * on `stream`; nothing is allocated; the workspace is the one
 * remap_groups_workspace(A.n_rows, A.nnz) sizes.
 *
 *   group_rid    (device) the 8-row schedule's row of every work slot
 *   share_meta   (device) 2 * (n_super + 1),  n_super = ceil(n_rows / (8 *
 *                share_waves)); slot 2 s = first union entry of supergroup s
 *   share_col, share_mask  (device) A.nnz + 256 each (union entries <= nnz;
 *                the 256 behind the last one are readable zeros)
 *   n_union_out  (device) one int64: union entries actually used
 */
REMAP_API int remap_share_build(const remap_csr *A, const int32_t *group_rid,
                      int32_t share_waves, int64_t *share_meta,
                      int32_t *share_col, int32_t *share_mask,
                      int64_t *n_union_out, void *workspace,
                      size_t workspace_bytes, void *stream);

/*
 * Build the LDS patch plan of kernel family 5 (remap_apply_args.patch_*) for
 * the rows of A on the device.  Work slots are walked in tile_y x tile_x
 * tiles of a 2-D destination grid (grid_dims = HOST {my, mx}; NULL: natural
 * order, patches of tile_y * tile_x consecutive rows); tile_y * tile_x
 * consecutive slots form a patch (= remap_apply_args.patch_rows).
 *
 *   row_order_out (device, A.n_rows; required with grid_dims)
 *   patch_ptr     (device) n_patches + 1      n_patches = ceil(n_rows / rows)
 *   patch_ucol    (device) A.nnz (distinct (patch, col) pairs <= nnz)
 *   patch_rowptr  (device) A.n_rows + 1
 *   patch_lidx, patch_val  (device) A.nnz
 *   stats_out     (device) int64[3]: distinct pairs, longest per-patch list
 *                 (patch_umax), most entries in one patch (patch_emax) --
 *                 what the caller needs to size the LDS image (see
 *                 patch_row_bytes) and to decide whether the tile fits
 * Asynchronous on `stream`; nothing is allocated.
 */
REMAP_API
int remap_patches_workspace(int64_t n_rows, int64_t nnz, size_t *bytes_out);
REMAP_API int remap_patches_build(const remap_csr *A, const int64_t *grid_dims,
                        int64_t row_offset, int32_t tile_y, int32_t tile_x,
                        int32_t *row_order_out, int32_t *patch_ptr,
                        int32_t *patch_ucol, int32_t *patch_rowptr,
                        int32_t *patch_lidx, double *patch_val,
                        int64_t *stats_out, void *workspace,
                        size_t workspace_bytes, void *stream);

/*
 * WHICH schedule a mapping gets -- decided (from the measurements recorded in
 * DESIGN.md section 6) and built in one call.  The schedule's arrays live in
 * ONE device arena the caller provides and keeps alive as long as the
 * schedule is used; the struct returns the ready-to-copy fields of
 * remap_apply_args.  Synchronous on `stream` (statistics are read back to
 * choose).  Query both sizes first with remap_schedule_sizes().
 *
 *   family  0: nothing to attach (no destination grid, empty matrix, or no
 *              source-row sharing to exploit)
 *           5: LDS patches   -> row_order, patch_*   (bilinear, coarse->fine)
 *          10: row groups    -> row_order, group_*   (conservative maps;
 *              entry-rich ones -- 2nd-order stencils -- also share_*)
 *           6: plain kernels in a tiled processing order -> row_order only
 *   tune[mode]: what to pass as remap_apply_args.tune for REMAP_MODE_<mode>,
 *              together with REMAP_FLAG_TUNE_HINT (a call the family cannot
 *              serve then falls back by itself)
 *   grid_dims  (HOST) the C-order dims of the WHOLE destination grid, n_dims
 *              = 1 or 2 (0: no grid, nothing is scheduled); row_offset = the
 *              index of A's first row in it (0 unless A is a row shard)
 */
typedef struct remap_schedule {
    int32_t family;
    int32_t entry_rich;          /* >= 10 entries per non-empty row          */
    const int32_t *row_order;    /* (device, arena) or NULL                  */
    const int32_t *patch_ptr;
    const int32_t *patch_ucol;
    const int32_t *patch_rowptr;
    const int32_t *patch_lidx;
    const double *patch_val;
    int32_t patch_rows;
    int32_t patch_umax;
    int32_t patch_emax;
    int32_t patch_row_bytes;
    int64_t n_patches;
    const int64_t *group_meta;
    const int32_t *group_col;
    const double *group_w;
    const int32_t *group_mask;
    const int32_t *group_rid;
    const double *group_frac;
    int64_t n_groups;
    int32_t group_rows;
    int32_t super_tile;          /* 0: groups row-major over the whole grid  */
    int32_t tile_y;              /* patch tile / processing-order tile       */
    int32_t tile_x;
    double ratio;                /* distinct/entries (5), union/entries (10) */
    int64_t n_distinct;          /* distinct pairs (5), union entries (10)   */
    int32_t tune[3][8];
    size_t arena_used;           /* bytes of the arena the schedule occupies */
    /* (ABI 25) entry-rich row groups: the shared union lists of the shared
     * form, remap_apply_args.share_* (NULL / 0 otherwise)                  */
    const int64_t *share_meta;
    const int32_t *share_col;
    const int32_t *share_mask;
    int32_t share_waves;
    int32_t share_reserved;
    int64_t n_share_union;       /* union entries of the supergroups        */
} remap_schedule;

REMAP_API
int remap_schedule_sizes(int64_t n_rows, int64_t nnz, size_t *arena_bytes,
                         size_t *workspace_bytes);
REMAP_API int remap_schedule_auto(const remap_csr *A, const double *frac_b,
                        const int64_t *grid_dims, int32_t n_dims,
                        int64_t row_offset, void *arena, size_t arena_bytes,
                        void *workspace, size_t workspace_bytes,
                        remap_schedule *schedule_out, void *stream);

/*
 * The whole path behind ONE opaque handle, device memory owned by the
 * library (hipMalloc / hipFree) -- for a binder without an allocator of its
 * own; the entry points above never allocate and suit a host layer that has
 * one (pyremap_amd keeps everything in torch tensors).
 *
 * remap_plan_create = `_load_mapping` (remap_numpy.py:72-139): the mapping
 *   file's triplets become the device CSR scipy would build (:134-137:
 *   sorted, duplicates summed), frac_b is copied, and the mapping gets its
 *   kernel schedule (remap_schedule_auto).  Cache the handle where the
 *   reference caches `remapper._matrix`.
 *     row, col (int32, `index_base`-based), S, frac_b: HOST arrays when
 *       host_input != 0 (the library uploads them), device arrays otherwise;
 *       not retained either way
 *     dst_grid_dims (HOST): C-order dims of the destination grid, n_dims =
 *       1 or 2 (0: no grid known -- the plain kernels)
 *   Synchronous on `stream`.  REMAP_ERR_ARG if a triplet is out of range.
 * remap_plan_apply = `_remap_numpy_array` (:223-297): one fused launch over
 *   all rows, asynchronous on `stream`; field layout and modes as in
 *   remap_apply_args (same names, same meaning).  (Two launches writing
 *   disjoint rows for a mapping whose few LONG rows -- more than 96 entries:
 *   the pole caps of a global bilinear map as ESMF makes it -- hold 2 % of
 *   the entries or more: remap_plan_create keeps those rows apart, see
 *   patch_ell_base.)
 *   The calling thread's current HIP device must be the one the plan was
 *   created on (REMAP_ERR_ARG otherwise: the launch would run against
 *   another device's pointers).
 * remap_plan_destroy frees the device memory on the plan's device, whatever
 *   device is current (the caller makes sure no launch still uses it).
 */
typedef struct remap_plan remap_plan;

typedef struct remap_plan_info {
    int64_t n_a;
    int64_t n_b;
    int64_t nnz;                 /* after duplicate summing                  */
    int64_t max_row_nnz;
    int32_t family;              /* remap_schedule.family chosen             */
    int32_t group_rows;
    double ratio;
    size_t device_bytes;         /* device memory the plan holds             */
    int32_t cell_patch_rows;     /* rows per patch of the lanes-across-rows
                                  * plan remap_plan_prepare_short_runs built
                                  * (0: not built)                           */
    int32_t reserved;
} remap_plan_info;

typedef struct remap_field {
    const void *X;               /* (device) source field                    */
    int32_t x_dtype;             /* REMAP_DTYPE_*                            */
    int32_t mode;                /* REMAP_MODE_* (REMAP_MODE_LAF and _MIN ..
                                  * _MEDIAN walk ONE CSR:
                                  * REMAP_ERR_UNSUPPORTED on a plan that
                                  * keeps its long rows apart)               */
    int64_t n_batch;
    int64_t k_inner;
    int64_t x_row_stride;        /* elements                                 */
    int64_t x_batch_stride;
    double *Y;                   /* (device) float64 result                  */
    int64_t y_row_stride;
    int64_t y_batch_stride;
    double threshold;            /* REMAP_MODE_MASKED, _LAF, _MIN .. _MEDIAN */
    uint8_t *mask_out;           /* (device) or NULL                         */
    const int32_t *gate;         /* (device) or NULL: see remap_apply_args   */
    int32_t gate_value;
    uint32_t flags;              /* REMAP_FLAG_FMA, REMAP_FLAG_TREE,
                                  * REMAP_FLAG_CELL_MASKS                    */
} remap_field;

REMAP_API int remap_plan_create(int64_t n_b, int64_t n_a, int64_t n_s,
                      const int32_t *row, const int32_t *col, const double *S,
                      int32_t index_base, const double *frac_b,
                      int32_t host_input, const int64_t *dst_grid_dims,
                      int32_t n_dims, void *stream, remap_plan **plan_out);
/*
 * Optional, once per plan, before fields whose contiguous run behind the
 * source axes is short and that come in several batches:
 *   (Time, nCells), MPAS's 2-D time series, the reference's most common
 *   input (tests/test_interpolate.py:57-59; k_inner < 4 and n_batch > 1):
 *   builds the patch plan of the LDS-staged lanes-across-rows kernel (32 x 32
 *   tiles of the destination grid -- 16 x 16 on grids under 128 K cells and
 *   on coarse-to-fine maps of fewer than 1 024 such tiles -- halved until
 *   no patch references more than 2 046 distinct source cells), which remap_plan_apply then uses for such
 *   fields.  Without it they take the unstaged lanes-across-rows kernel
 *   (2.5 x slower on EC30to60 -> 0.5 degree at Time = 120);
 *   (Time, nCells, 4 ... 15 levels) on mappings scheduled as row groups:
 *   two more patch plans -- 16 x 16 tiles for the batch-at-a-time kernel
 *   (4 ... 6 levels), 4 x 8 tiles for the LDS patch kernel (7 ... 15) --
 *   1.3-1.9 x faster than the row groups on such runs.
 * Each plan takes 16 bytes per entry of the mapping.  Allocates device
 * memory (remap_plan_apply never does) and synchronises `stream`; a second
 * call does nothing.
 */
REMAP_API int remap_plan_prepare_short_runs(remap_plan *plan, void *stream);
REMAP_API void remap_plan_destroy(remap_plan *plan);
REMAP_API
int remap_plan_query(const remap_plan *plan, remap_plan_info *info_out);
REMAP_API
int remap_plan_apply(const remap_plan *plan, const remap_field *field,
                     void *stream);

/*
 * `_remap_data_array` in one call (remap_numpy.py:201-204 + :223-297): scan
 * the field for NaNs on the device and enqueue the masked, renormalised
 * branch (threshold = field->threshold) and the frac_b branch, each gated on
 * what the scan finds -- nothing synchronises, nothing is allocated, the
 * sequence is hipGraph-capturable.  What is scanned is what the call reads:
 * the n_a cells x n_batch x k_inner values the field's strides address
 * (`x_elems` is kept for callers of ABI 24 and only checked for sign);
 * `field->mode` and `field->gate` are ignored; `kinds` is a device int32[4]
 * (ABI 25: two more words) the call zeroes and fills (see
 * remap_scan_nan_layout).  On a mapping scheduled as 8-row groups the masked
 * branch is enqueued in each of its forms (REMAP_FLAG_CELL_MASKS,
 * REMAP_FLAG_BATCH_MASKS, neither): four gated launches instead of two.
 */
REMAP_API
int remap_plan_apply_auto(const remap_plan *plan, const remap_field *field,
                          int64_t x_elems, int32_t *kinds, void *stream);

/*
 * OR 1 into *flag (device int32, zeroed by the caller) if any of the n
 * elements of x (device, REMAP_DTYPE_*, element-aligned) is a NaN.
 * Asynchronous on `stream`; the device half of remap_numpy.py:201-204.
 */
REMAP_API
int remap_scan_nan(const void *x, int32_t x_dtype, int64_t n, int32_t *flag,
                   void *stream);

/*
 * remap_scan_nan() with the KIND of the missing values (device int32[2],
 * zeroed by the caller): kinds[0] |= 1 if x holds a NaN (what
 * remap_scan_nan() reports); kinds[1] |= 1 if x holds a NaN, |= 2 if some
 * aligned run of 16 bytes x 64 lanes (128 float64 / 256 float32 elements in
 * memory order) holds NaNs AND numbers -- so kinds[1] is 0 (no NaN), 1 (NaNs
 * in whole runs: whole cells of an (n_a, K) field missing) or 3 (NaNs
 * column by column).  Three gated calls then cover remap_numpy.py:201-204
 * on an entry-rich mapping: FRACB gated on kinds[0] == 0, MASKED with
 * REMAP_FLAG_CELL_MASKS gated on kinds[1] == 1, MASKED without it gated on
 * kinds[1] == 3.  A hint only: results never depend on it.
 */
REMAP_API int remap_scan_nan_kinds(const void *x, int32_t x_dtype, int64_t n,
                         int32_t *kinds, void *stream);

/*
 * The scan with the field's LAYOUT (ABI 25; device int32[4], zeroed by the
 * caller): source cell a's k_inner values of batch b lie at x[b *
 * x_batch_stride + a * x_row_stride + k], as in remap_apply_args.  What is
 * missing is judged per source cell and per batch -- where the cells and the
 * batches are, not in aligned runs of memory, which a (Time, nCells,
 * nVertLevels) field with land cells reads as "column by column":
 *   kinds[0]  1 if the field holds a NaN
 *   kinds[1]  0 no NaN; 1 every cell is missing in ALL of its n_batch *
 *             k_inner columns or in none (land: what REMAP_FLAG_CELL_MASKS
 *             expects); 3 otherwise
 *   kinds[2]  0 no NaN; 1 every batch has the mask of batch 0 (bathymetry:
 *             what REMAP_FLAG_BATCH_MASKS expects); 3 otherwise
 *   kinds[3]  the launch that suits: 0 none (FRACB), 1 MASKED with
 *             REMAP_FLAG_CELL_MASKS, 2 MASKED with REMAP_FLAG_BATCH_MASKS
 *             (n_batch >= 3 only), 3 MASKED without either
 * Four calls gated on kinds[3] == 0 / 1 / 2 / 3 then cover
 * remap_numpy.py:201-204 on an entry-rich mapping without a host round
 * trip.  Hints only: results never depend on them.  Asynchronous on
 * `stream`; kinds[3] is written by a second small launch behind the scan.
 */
REMAP_API int remap_scan_nan_layout(const void *x, int32_t x_dtype,
                          int64_t n_rows, int64_t n_batch, int64_t k_inner,
                          int64_t x_row_stride, int64_t x_batch_stride,
                          int32_t *kinds, void *stream);

/*
 * The two device steps of a ROW SHARD's exchange (no counterpart in the
 * reference, which is single-process; the math is remap_numpy.py:264-268:
 * destination row i reads only the source rows its entries name, so a shard
 * of rows needs X[unique(col[shard])] and nothing else -- whatever the
 * numbering of the source mesh).
 *
 * remap_pack_columns: one-off per shard.  ucols_out (device, capacity
 *   min(nnz, n_cols)) receives the DISTINCT column indices of `col`
 *   ascending, *n_ucols_out (device int64) their number, and col_out (device,
 *   nnz; may alias col) the same entries renumbered to positions in that
 *   list.  The renumbering is monotone: a row's entries keep their order, so
 *   the packed shard reproduces the unsharded result bit for bit.
 *   *bad_out (device int64) counts entries outside [0, n_cols).
 * remap_gather_rows: per batch of fields, on the device that holds them:
 *   dst[b][i][0:row_bytes] = src[b * batch_stride + rows[i] * row_stride ...]
 *   for b < n_batch, i < n_rows; dst is contiguous (n_batch, n_rows,
 *   row_bytes).  With rows = a shard's ucols this is the packed source
 *   buffer that travels to the shard's GPU; strides in BYTES.
 * Both asynchronous on `stream`; nothing is allocated.
 */
REMAP_API int remap_pack_columns_workspace(int64_t n_cols, size_t *bytes_out);
REMAP_API
int remap_pack_columns(const int32_t *col, int64_t nnz, int64_t n_cols,
                       int32_t *col_out, int32_t *ucols_out,
                       int64_t *n_ucols_out, int64_t *bad_out,
                       void *workspace, size_t workspace_bytes, void *stream);
REMAP_API int remap_gather_rows(const void *src, int64_t n_batch,
                      int64_t src_batch_stride_bytes,
                      int64_t src_row_stride_bytes, const int32_t *rows,
                      int64_t n_rows, int64_t row_bytes, void *dst,
                      void *stream);

/*
 * Device-to-device streaming copy of `bytes` (16 B per lane, grid-stride):
 * the box's achievable HBM ceiling, reported beside the roofline numbers.
 */
REMAP_API
int remap_stream_copy(void *dst, const void *src, size_t bytes, void *stream);

/*
 * The shader clock the chip holds right now (asynchronous on `stream`): one
 * wave spins for `micros` microseconds (1 ... 1000) and writes the shader
 * cycles (s_memtime) and the constant-rate 100 MHz ticks (s_memrealtime) it
 * saw go by to ticks_out[0] / ticks_out[1] (device, 2 x int64): MHz = 100 *
 * ticks_out[0] / ticks_out[1].  Queued right behind a series of launches it
 * tells which clock state their times belong to (an instruction-issue-bound
 * kernel such as the LDS patch kernel runs 5.2 or 6.4 ms per launch on
 * config 4 depending on it).  Measurement only.
 */
REMAP_API
int remap_clock_probe(int64_t *ticks_out, int32_t micros, void *stream);

/*
 * ---------------------------------------------------------------------------
 * Conservative overlaps between an MPAS cell mesh and a lat-lon grid (an
 * addition: the reference has ESMF_RegridWeightGen --method conserve compute
 * them, pyremap/remapper/build_map.py).  ESMF's geometry: every cell is a
 * spherical polygon with great-circle edges, lat-lon cells included (their
 * corners joined by great-circle arcs; a polar row's cells are triangles).
 * The overlap list is what both directions of a first-order conservative map
 * are made of (pyremap_amd/weights.py turns it into S and frac_b).
 *
 * Call remap_overlap_latlon_sizes() first: it counts the candidate pairs
 * (mesh cell, lat-lon cell whose boxes meet) on `stream` and reads the count
 * back (it synchronises `stream`), and returns it with the workspace size.
 * remap_overlap_latlon() is then asynchronous on `stream` except for ONE
 * host read-back: the number of entries (and the error bits) after the
 * clipping, before the sort.  No floating-point atomics: two calls give
 * bitwise-identical outputs.
 * ---------------------------------------------------------------------------
 */

/* the largest nEdgesOnCell this build serves (clip polygons live in LDS) */
#define REMAP_OVERLAP_MAX_EDGES 10

/* error bits behind a REMAP_ERR_UNSUPPORTED of the overlap calls */
enum {
    REMAP_OVERLAP_ERR_EDGES = 1,      /* nEdgesOnCell > REMAP_OVERLAP_MAX_EDGES */
    REMAP_OVERLAP_ERR_VERTEX = 2,     /* < 3 distinct vertices, bad index      */
    REMAP_OVERLAP_ERR_HEMISPHERE = 4, /* a pair's vertex within acos(0.1) of
                                         the horizon of the mesh cell's centre
                                         (the gnomonic projection's limit)     */
    REMAP_OVERLAP_ERR_CAPACITY = 8,   /* n_pairs differs from the count        */
    REMAP_OVERLAP_ERR_CONVEX = 32     /* a clipper cell (b of remap_overlap_meshes
                                         / _grids) is not convex              */
};

typedef struct remap_overlap_geom {
    int64_t n_cells;            /* mesh cells (nCells)                        */
    int64_t n_vertices;         /* mesh vertices (nVertices)                  */
    int64_t n_lat;              /* grid rows                                  */
    int64_t n_lon;              /* grid columns; grid cell = row * n_lon + col */
    int32_t max_edges;          /* maxEdges: the row stride of verticesOnCell */
    int32_t reserved;           /* 0                                          */
    /* how far north (south) of its corners' latitude a grid cell's
     * great-circle edge reaches, at most over the grid, radians; candidate
     * rows are widened by it */
    double lat_slack;
    const int32_t *vertices_on_cell; /* (device) n_cells x max_edges, 1-based */
    const int32_t *n_edges_on_cell;  /* (device) n_cells                      */
    const double *lat_vertex;   /* (device) n_vertices, radians               */
    const double *lon_vertex;   /* (device) n_vertices, radians               */
    const double *lat_corner;   /* (device) n_lat + 1, radians, monotone,
                                   within [-pi/2, pi/2]                       */
    const double *lon_corner;   /* (device) n_lon + 1, radians, monotone; a
                                   grid spanning 2 pi closes in longitude     */
} remap_overlap_geom;

/*
 *   counter (device) 2 x int64 of scratch;  n_pairs_out (host) candidate
 *   pairs;  workspace_bytes_out (host) what remap_overlap_latlon() needs.
 */
REMAP_API
int remap_overlap_latlon_sizes(const remap_overlap_geom *geom,
                               int64_t *counter, int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream);

/*
 * The overlap areas A (steradians) of every (destination, source) pair with
 * A > 1e-14 x area(destination cell), sorted by (dst, src), 0-based.  The
 * destination is the mesh when dst_is_mesh != 0, the grid otherwise.
 *
 *   dst_out, src_out, area_out (device) n_pairs capacity each, the first
 *   *n_entries_out meaningful;  frac_b_out (device) one per destination
 *   cell: min(sum of its entries / its area, 1), summed in entry order;
 *   mesh_area_out (device) n_cells, grid_area_out (device) n_lat x n_lon:
 *   the polygons' own areas;  n_entries_out (host) one int64.
 */
REMAP_API
int remap_overlap_latlon(const remap_overlap_geom *geom, int32_t dst_is_mesh,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *mesh_area_out,
                         double *grid_area_out, int64_t *n_entries_out,
                         void *stream);

/*
 * ---------------------------------------------------------------------------
 * Conservative overlaps between two MPAS cell meshes a and b (the same
 * geometry, normalisation and sliver rule as remap_overlap_latlon).  Cells of
 * b are found for each cell of a through a global uniform lat-lon raster of
 * buckets sized to b; every candidate (a, b) pair is clipped once, a's
 * polygon by b's (b's cells must be convex: REMAP_OVERLAP_ERR_CONVEX), so
 * both directions (dst_is_b) give the same overlap list, transposed, with
 * the same bits.
 *
 * remap_overlap_meshes_sizes() counts the candidate pairs and reads the
 * count back (it synchronises `stream`, and allocates and frees device
 * memory of one int32 per bucket).  remap_overlap_meshes() is then
 * asynchronous on `stream` except for TWO host read-backs: the bucket key
 * counts (and the cells' error bits) after the cell preparation, and the
 * number of entries (and the remaining error bits) before the sort.  No
 * floating-point atomics: two calls give bitwise-identical outputs.
 * ---------------------------------------------------------------------------
 */
typedef struct remap_overlap_mesh {
    int64_t n_cells;            /* nCells                                     */
    int64_t n_vertices;         /* nVertices                                  */
    int32_t max_edges;          /* maxEdges: the row stride of verticesOnCell */
    int32_t reserved;           /* 0                                          */
    const int32_t *vertices_on_cell; /* (device) n_cells x max_edges, 1-based */
    const int32_t *n_edges_on_cell;  /* (device) n_cells                      */
    const double *lat_vertex;   /* (device) n_vertices, radians               */
    const double *lon_vertex;   /* (device) n_vertices, radians               */
} remap_overlap_mesh;

/*
 *   counter (device) 4 x int64 of scratch;  n_pairs_out (host) candidate
 *   pairs;  workspace_bytes_out (host) what remap_overlap_meshes() needs.
 */
REMAP_API
int remap_overlap_meshes_sizes(const remap_overlap_mesh *a,
                               const remap_overlap_mesh *b, int64_t *counter,
                               int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream);

/*
 * The overlap areas A (steradians) of every (destination, source) pair with
 * A > 1e-14 x area(destination cell), sorted by (dst, src), 0-based.  The
 * destination is mesh b when dst_is_b != 0, mesh a otherwise.
 *
 *   dst_out, src_out, area_out (device) n_pairs capacity each, the first
 *   *n_entries_out meaningful;  frac_b_out (device) one per destination
 *   cell: min(sum of its entries / its area, 1), summed in entry order;
 *   a_area_out (device) a->n_cells, b_area_out (device) b->n_cells: the
 *   polygons' own areas;  n_entries_out (host) one int64.
 */
REMAP_API
int remap_overlap_meshes(const remap_overlap_mesh *a,
                         const remap_overlap_mesh *b, int32_t dst_is_b,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *a_area_out,
                         double *b_area_out, int64_t *n_entries_out,
                         void *stream);

/*
 * ---------------------------------------------------------------------------
 * Conservative overlaps between two polygon soups whose cells come in convex
 * PIECES (the cells of an MPAS vertex mesh beside a land mask are concave;
 * any cell can be handed over as triangles).  Each side is a mesh of pieces
 * and, per piece, the cell it belongs to.  The geometry, the candidate
 * search (bucket raster sized to b), the clip and the error bits are those
 * of remap_overlap_meshes applied to the pieces: every piece of b must be
 * convex (REMAP_OVERLAP_ERR_CONVEX), pieces of a are subjects.  The outputs
 * are in CELLS: A(dst cell, src cell) is the sum of the areas of its piece
 * pairs, added in ascending (dst piece, src piece) order; a cell's area is
 * the sum of its pieces' areas in piece order; the sliver rule (A > 1e-14 x
 * area(dst cell)) applies to the merged sum; frac_b = min(sum of the
 * entries / area, 1) in entry order; entries sorted by (dst, src), unique.
 * No floating-point atomics: two calls give bitwise-identical outputs, and
 * with parent == NULL on both sides every output has the bytes
 * remap_overlap_meshes gives.
 *
 * REMAP_ERR_ARG: a parent array that decreases, leaves [0, n_parents) or
 * skips a cell (a cell without a piece), n_parents > 2^31 - 1, n_parents
 * that cannot match the pieces.  Host read-backs: those of
 * remap_overlap_meshes, one for the parents' check (none with NULL parents)
 * and one for the entry count behind the merge.
 * ---------------------------------------------------------------------------
 */
/* (a struct tag, not a typedef: the name is also the call's) */
struct remap_overlap_pieces {
    remap_overlap_mesh mesh;    /* the PIECES, as cells of a mesh            */
    int64_t n_parents;          /* cells the pieces belong to                */
    const int32_t *parent;      /* (device) mesh.n_cells, 0-based, non-
                                   decreasing; NULL: piece k is cell k       */
};

/*
 *   counter (device) 4 x int64 of scratch;  n_pairs_out (host) candidate
 *   piece pairs;  workspace_bytes_out (host) what remap_overlap_pieces()
 *   needs.
 */
REMAP_API
int remap_overlap_pieces_sizes(const struct remap_overlap_pieces *a,
                               const struct remap_overlap_pieces *b, int64_t *counter,
                               int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream);

/*
 *   dst_out, src_out, area_out (device) n_pairs capacity each, the first
 *   *n_entries_out meaningful, indices of CELLS;  frac_b_out (device) one per
 *   destination cell;  a_area_out (device) a->n_parents, b_area_out (device)
 *   b->n_parents: the cells' areas;  n_entries_out (host) one int64.
 */
REMAP_API
int remap_overlap_pieces(const struct remap_overlap_pieces *a,
                         const struct remap_overlap_pieces *b, int32_t dst_is_b,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *a_area_out,
                         double *b_area_out, int64_t *n_entries_out,
                         void *stream);

/*
 * The same call for measurements: phase_ms_out (host) receives 5 floats, the
 * GPU milliseconds of the cell preparation, the candidate pairs, the clip
 * (with its compaction), the sort and the merge (with frac_b), from events
 * on `stream`; it synchronises the stream before it returns.
 */
REMAP_API
int remap_overlap_pieces_timed(const struct remap_overlap_pieces *a,
                               const struct remap_overlap_pieces *b,
                               int32_t dst_is_b, int64_t n_pairs,
                               void *workspace, size_t workspace_bytes,
                               int32_t *dst_out, int32_t *src_out,
                               double *area_out, double *frac_b_out,
                               double *a_area_out, double *b_area_out,
                               int64_t *n_entries_out, float *phase_ms_out,
                               void *stream);

/*
 * ---------------------------------------------------------------------------
 * Conservative overlaps where at least one side is a structured 2-D grid
 * given by its corner arrays (the same geometry, normalisation and sliver
 * rule as remap_overlap_latlon).  A side is an MPAS cell mesh or a grid of
 * ny x nx cells; grid cell j * nx + i is the spherical polygon through the
 * corners (j, i), (j, i + 1), (j + 1, i + 1), (j + 1, i), great-circle edges,
 * consecutive equal corners dropped (a cell may be a triangle), either
 * orientation.  Side a's polygons are clipped by side b's (b's cells must be
 * convex: REMAP_OVERLAP_ERR_CONVEX); both directions (dst_is_b) give the same
 * overlap list, transposed, with the same bits.
 *
 * Candidates come from a pyramid of bounding caps over the grid's own
 * ny x nx index space (2 x 2 nodes per node), walked once per cell of the
 * other side; when both sides are grids the pyramid is b's.  Nothing but the
 * corner arrays is needed: a pole inside the grid and cells across the
 * longitude seam are served.  A grid has at most 16384 cells a side.
 *
 * remap_overlap_grids_sizes() prepares both sides and counts the candidate
 * pairs in device memory of its own (it allocates and frees it, and
 * synchronises `stream`).  remap_overlap_grids() is then asynchronous on
 * `stream` except for ONE host read-back: the number of entries (and every
 * error bit) after the clipping, before the sort.  No floating-point
 * atomics: two calls give bitwise-identical outputs.
 * ---------------------------------------------------------------------------
 */
typedef struct remap_overlap_grid {
    int64_t ny;                 /* cell rows                                  */
    int64_t nx;                 /* cell columns                               */
    const double *lat_corner;   /* (device) (ny + 1) x (nx + 1), C order,
                                   radians, within [-pi/2, pi/2]              */
    const double *lon_corner;   /* (device) (ny + 1) x (nx + 1), radians, any
                                   branch                                     */
} remap_overlap_grid;

/* one side: exactly one of the two is non-NULL */
typedef struct remap_overlap_side {
    const remap_overlap_mesh *mesh;
    const remap_overlap_grid *grid;
} remap_overlap_side;

/*
 *   n_pairs_out (host) candidate pairs;  workspace_bytes_out (host) what
 *   remap_overlap_grids() needs.  At least one side must be a grid.
 */
REMAP_API
int remap_overlap_grids_sizes(const remap_overlap_side *a,
                              const remap_overlap_side *b,
                              int64_t *n_pairs_out,
                              size_t *workspace_bytes_out, void *stream);

/*
 * The overlap areas A (steradians) of every (destination, source) pair with
 * A > 1e-14 x area(destination cell), sorted by (dst, src), 0-based.  The
 * destination is side b when dst_is_b != 0, side a otherwise.
 *
 *   dst_out, src_out, area_out (device) n_pairs capacity each, the first
 *   *n_entries_out meaningful;  frac_b_out (device) one per destination
 *   cell: min(sum of its entries / its area, 1), summed in entry order;
 *   a_area_out, b_area_out (device) one per cell of a / b: the polygons'
 *   own areas;  n_entries_out (host) one int64.
 */
REMAP_API
int remap_overlap_grids(const remap_overlap_side *a,
                        const remap_overlap_side *b, int32_t dst_is_b,
                        int64_t n_pairs, void *workspace,
                        size_t workspace_bytes, int32_t *dst_out,
                        int32_t *src_out, double *area_out,
                        double *frac_b_out, double *a_area_out,
                        double *b_area_out, int64_t *n_entries_out,
                        void *stream);

/*
 * ---------------------------------------------------------------------------
 * Nearest source point of every destination point: ESMF's `neareststod`.
 * src_xyz (n_src, 3) and dst_xyz (n_dst, 3) are fp64, finite, C order (unit
 * vectors for points on the sphere, but nothing assumes it).  For destination
 * i and source j
 *     dx = src[j].x - dst[i].x   (likewise y, z)
 *     d2(i, j) = (dx * dx + dy * dy) + dz * dz
 * in IEEE fp64 in that order, no contraction, and nearest_out[i] is the j
 * (0-based) that minimises (d2(i, j), j) lexicographically: the smallest
 * distance, and among equal d2 bit patterns the lowest source index.  Exact:
 * the result is a pure function of the inputs, whatever their distribution
 * (regional sources, clusters, duplicates, any numbering).
 *
 * The sources are sorted by a Morton code (rocPRIM radix sort), a tree of
 * axis-aligned boxes is built over the sorted array (8 points a leaf, 4
 * nodes a node) and walked depth first by one lane per destination point;
 * a node is skipped only when its bound -- d2's own formula on the distance
 * to the box, which never exceeds the d2 of a point inside -- is STRICTLY
 * greater than the best d2 so far, so ties survive.  No atomics: two calls
 * give identical bytes.  Everything is asynchronous on `stream`, nothing is
 * read back; the workspace depends on (n_src, n_dst) alone.
 *
 *   REMAP_ERR_ARG        a NULL array, n_src < 1, n_dst < 0, n_src > 2^31 - 1
 *   REMAP_ERR_WORKSPACE  workspace_bytes below remap_nearest_workspace()'s
 *   n_dst == 0           REMAP_OK, nothing is launched
 * ---------------------------------------------------------------------------
 */
/*
 * Launches nothing and touches no device memory; the size of rocPRIM's sort
 * buffer is asked of rocPRIM, which may look up the current device's
 * properties to choose its configuration (as remap_csr_from_coo_workspace
 * and remap_groups_workspace do): call it with the device current that
 * remap_nearest() will run on.
 */
REMAP_API
int remap_nearest_workspace(int64_t n_src, int64_t n_dst, size_t *bytes_out);

/*
 *   src_xyz, dst_xyz, nearest_out, workspace (device);  nearest_out one
 *   int32 per destination point.
 */
REMAP_API
int remap_nearest(const double *src_xyz, int64_t n_src, const double *dst_xyz,
                  int64_t n_dst, int32_t *nearest_out, void *workspace,
                  size_t workspace_bytes, void *stream);

/*
 * remap_nearest() for measurements: the same launches with events between
 * the phases.  This one WAITS for the last event, then writes
 * phase_ms_out[0..2] (host): milliseconds of keys + sort + gather, of the
 * boxes, and of the walk.  (With n_dst == 0 the first two phases still run.)
 */
REMAP_API
int remap_nearest_timed(const double *src_xyz, int64_t n_src,
                        const double *dst_xyz, int64_t n_dst,
                        int32_t *nearest_out, void *workspace,
                        size_t workspace_bytes, float *phase_ms_out,
                        void *stream);

/*
 * ---------------------------------------------------------------------------
 * The k nearest source points of every destination point: the search behind
 * ESMF's `--extrap_method neareststod | nearestidavg`.  Inputs and d2 as for
 * remap_nearest() above.  Row i of idx_out / d2_out, both (n_dst, k) in C
 * order, holds the min(k, n_src) sources that come first in (d2(i, j), j)
 * lexicographic order, ascending: 0-based index and d2.  The slots behind
 * them (k > n_src) hold index -1 and d2 = +inf.  Exact, a pure function of
 * the inputs; k = 1 gives remap_nearest()'s indices.
 *
 * The same sort and tree; the walk keeps each lane's k best in LDS beside
 * its stack and skips a box only when its bound is STRICTLY greater than the
 * k-th best d2 so far (never while fewer than k are held).  No atomics: two
 * calls give identical bytes.  Asynchronous on `stream`, nothing is read
 * back; the workspace is remap_nearest()'s, whatever k.
 *
 *   REMAP_ERR_ARG        a NULL array, n_src < 1, n_dst < 0, n_src > 2^31 - 1,
 *                        k outside 1 .. REMAP_NEAREST_K_MAX
 *   REMAP_ERR_WORKSPACE  workspace_bytes below remap_nearest_k_workspace()'s
 *   n_dst == 0           REMAP_OK, nothing is launched
 * ---------------------------------------------------------------------------
 */
#define REMAP_NEAREST_K_MAX 16

/* (as remap_nearest_workspace: call it with the device current that
 * remap_nearest_k() will run on) */
REMAP_API
int remap_nearest_k_workspace(int64_t n_src, int64_t n_dst, int32_t k,
                              size_t *bytes_out);

/*
 *   src_xyz, dst_xyz, idx_out, d2_out, workspace (device)
 */
REMAP_API
int remap_nearest_k(const double *src_xyz, int64_t n_src,
                    const double *dst_xyz, int64_t n_dst, int32_t k,
                    int32_t *idx_out, double *d2_out, void *workspace,
                    size_t workspace_bytes, void *stream);

/*
 * ---------------------------------------------------------------------------
 * Point location in spherical triangles: the search behind `bilinear` maps
 * from an MPAS mesh (the triangles of its dual mesh).  xyz (n_nodes, 3) fp64,
 * tri (n_tri, 3) int32 node ids (0-based), points (n_pts, 3) fp64, all C
 * order; nodes and points are unit vectors to within 1e-6; tol >= 0.  With
 *     cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
 *     dot(u, v)   = (u.x*v.x + u.y*v.y) + u.z*v.z
 * in IEEE fp64 in that order, no contraction, for the triangle t = (a, b, c)
 * and the point q
 *     D = dot(a, cross(b, c)),  s = -1 if D < 0, else +1
 *     w0 = s*dot(q, cross(b, c)),  w1 = s*dot(q, cross(c, a)),
 *     w2 = s*dot(q, cross(a, b)),  tot = (w0 + w1) + w2
 *     holds(q, t)  iff  tot > 0 and every w_k >= -tol*tot
 * A triangle with D == 0, D not finite or a node id outside [0, n_nodes)
 * holds nothing and is never dereferenced.  found_out[q] is the LOWEST t that
 * holds q, or -1; weights_out[q] are the winner's S_k = v_k / ((v0 + v1) +
 * v2) with v_k = w_k > 0 ? w_k : 0.0, zeros where found_out[q] is -1.  Exact:
 * a pure function of the inputs, whatever the triangles' orientation, order
 * or sizes (a variable-resolution mesh, overlapping triangles, duplicates).
 *
 * The triangles are sorted by the Morton code of their centroids (rocPRIM
 * radix sort), a tree of axis-aligned boxes is built over the sorted array
 * (8 triangles a leaf, 4 nodes a node) and walked depth first by one lane
 * per point.  A triangle's box is the box of its corners widened by a margin
 * of its own that covers the sphere's bulge over the flat triangle, the 1e-6
 * and tol (pyremap_amd/csrc/remap_locate.hip has the derivation): a triangle
 * is skipped only where holds() rejects the point.  No atomics: two calls
 * give identical bytes.  Everything is asynchronous on `stream`, nothing is
 * read back; the workspace depends on (n_nodes, n_tri, n_pts) alone.  Inputs
 * outside the unit-vector contract give an unspecified result; the call
 * still ends and stays inside its arrays.
 *
 *   REMAP_ERR_ARG        a NULL array, n_nodes < 1, n_tri < 1, n_tri >
 *                        2^31 - 1, n_pts < 0, tol < 0 or NaN
 *   REMAP_ERR_WORKSPACE  workspace_bytes below remap_locate_workspace()'s
 *   n_pts == 0           REMAP_OK, nothing is launched
 * ---------------------------------------------------------------------------
 */
/*
 * Launches nothing and touches no device memory (rocPRIM is asked for its
 * sort buffer, as in remap_nearest_workspace: call it with the device current
 * that remap_locate() will run on).
 */
REMAP_API
int remap_locate_workspace(int64_t n_nodes, int64_t n_tri, int64_t n_pts,
                           size_t *bytes_out);

/*
 *   xyz, tri, points, found_out, weights_out, workspace (device);  found_out
 *   one int32 and weights_out three doubles per point.
 */
REMAP_API
int remap_locate(const double *xyz, int64_t n_nodes, const int32_t *tri,
                 int64_t n_tri, const double *points, int64_t n_pts,
                 double tol, int32_t *found_out, double *weights_out,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * remap_locate() for measurements: the same launches with events between the
 * phases.  This one WAITS for the last event, then writes phase_ms_out[0..2]
 * (host): milliseconds of keys + sort, of normals + boxes, and of the walk.
 * (With n_pts == 0 the first two phases still run.)
 */
REMAP_API
int remap_locate_timed(const double *xyz, int64_t n_nodes, const int32_t *tri,
                       int64_t n_tri, const double *points, int64_t n_pts,
                       double tol, int32_t *found_out, double *weights_out,
                       void *workspace, size_t workspace_bytes,
                       float *phase_ms_out, void *stream);

/*
 * ---------------------------------------------------------------------------
 * Point location in the quads between four neighbouring cell centres: the
 * search behind `bilinear` maps from a grid given by 2-D latitude /
 * longitude arrays.  nodes (ny, nx, 3) fp64 unit vectors of the centres (C
 * order), ny >= 2, nx >= 2; periodic 0 or 1 (with 1 column nx-1 closes onto
 * column 0); points (n_pts, 3) fp64; nodes and points are unit vectors to
 * within 1e-6; tol >= 0.  nqx = nx - 1 + periodic, and quad k = j*nqx + i has
 * the corners p0 = (j, i), p1 = (j, i1), p2 = (j+1, i1), p3 = (j+1, i),
 * i1 = (i+1) % nx.  With cross and dot as above, in IEEE fp64 in that order,
 * no contraction, component by component
 *     c0 = 0.25*(((p0+p1)+p2)+p3)      c1 = 0.25*(((p1-p0)+p2)-p3)
 *     c2 = 0.25*(((p2-p0)-p1)+p3)      c3 = 0.25*(((p0-p1)+p2)-p3)
 * and Newton on c0 + s*c1 + t*c2 + s*t*c3 = r*q from s = t = 0, r = 1, at
 * most 12 steps, each
 *     F = (((c0 + s*c1) + t*c2) + (s*t)*c3) - r*q
 *     a = c1 + t*c3,  b = c2 + s*c3,  bq = cross(b, q),  det = -dot(a, bq)
 *     d0 = dot(F, bq)/det,  d1 = dot(a, cross(F, q))/det,
 *     d2 = -dot(a, cross(b, F))/det;   s += d0, t += d1, r += d2
 *     !(|s| <= 50) or !(|t| <= 50): the quad holds nothing
 *     an earlier step had max(|d0|, |d1|) <= 1e-8: the solve is done (this
 *     step was the polish); otherwise such a step asks for exactly one more
 * (not done after 12 steps: the quad holds nothing),
 *     holds(q, k)  iff  done, |s| <= 1 + tol, |t| <= 1 + tol and r > 0.
 * A quad with a non-finite corner holds nothing.  found_out[q] is the LOWEST
 * k that holds q, or -1; weights_out[q] are, with s and t clipped to [-1, 1],
 * 0.25*(1-s)*(1-t), 0.25*(1+s)*(1-t), 0.25*(1+s)*(1+t), 0.25*(1-s)*(1+t) for
 * p0..p3, zeros where found_out[q] is -1.  Exact: a pure function of the
 * inputs, whatever the grid's orientation or refinement, overlapping and
 * collapsed quads included.
 *
 * The quads are sorted by the Morton code of c0 (rocPRIM radix sort), a tree
 * of axis-aligned boxes is built over the sorted array (8 quads a leaf, 4
 * nodes a node) and walked depth first by one lane per point.  A quad's box
 * is the box of its corners widened by a margin of its own that covers the
 * sphere's bulge over the patch, the 1e-6 and tol; a quad too flat or folded
 * for that bound is tested against every point
 * (pyremap_amd/csrc/remap_quads.hip has the derivation): a quad is skipped
 * only where holds() rejects the point.  No atomics: two calls give identical
 * bytes.  Everything is asynchronous on `stream`, nothing is read back; the
 * workspace depends on (ny, nx, periodic, n_pts) alone.  Inputs outside the
 * unit-vector contract give an unspecified result; the call still ends and
 * stays inside its arrays.
 *
 *   REMAP_ERR_ARG        a NULL array, ny < 2, nx < 2, more than 2^31 - 1
 *                        quads, periodic not 0 or 1, n_pts < 0, tol < 0 or
 *                        NaN
 *   REMAP_ERR_WORKSPACE  workspace_bytes below remap_quads_workspace()'s
 *   n_pts == 0           REMAP_OK, nothing is launched
 * ---------------------------------------------------------------------------
 */
/*
 * Launches nothing and touches no device memory (rocPRIM is asked for its
 * sort buffer: call it with the device current that remap_quads() will run
 * on).
 */
REMAP_API
int remap_quads_workspace(int64_t ny, int64_t nx, int32_t periodic,
                          int64_t n_pts, size_t *bytes_out);

/*
 *   nodes, points, found_out, weights_out, workspace (device);  found_out
 *   one int32 and weights_out four doubles per point.
 */
REMAP_API
int remap_quads(const double *nodes, int64_t ny, int64_t nx, int32_t periodic,
                const double *points, int64_t n_pts, double tol,
                int32_t *found_out, double *weights_out, void *workspace,
                size_t workspace_bytes, void *stream);

/*
 * remap_quads() for measurements: the same launches with events between the
 * phases.  This one WAITS for the last event, then writes phase_ms_out[0..2]
 * (host): milliseconds of keys + sort, of coefficients + boxes, and of the
 * walk.  (With n_pts == 0 the first two phases still run.)
 */
REMAP_API
int remap_quads_timed(const double *nodes, int64_t ny, int64_t nx,
                      int32_t periodic, const double *points, int64_t n_pts,
                      double tol, int32_t *found_out, double *weights_out,
                      void *workspace, size_t workspace_bytes,
                      float *phase_ms_out, void *stream);

/*
 * ---------------------------------------------------------------------------
 * Cells widened about their centres: the reference's expand_dist /
 * expand_factor, applied to the DESTINATION cells of a smoothed `conserve`
 * map before their overlaps are taken.  centre_lat / centre_lon (n_cells),
 * corner_lat / corner_lon (n_cells, width) row-major, radians; the first
 * count[i] slots of row i are corners, 0 <= count[i] <= width.  dist (metres)
 * and factor are read at [i * stride], stride 0 (one value for every cell)
 * or 1 (a value per cell).  All fp64, IEEE, no contraction, on WGS84
 * (a = 6378137 m, 1/f = 298.257223563, b = a (1 - f), e2 = f (2 - f),
 * e'2 = e2 / (1 - e2)) at height 0:
 *     ecef(lat, lon) = (N cos lat cos lon, N cos lat sin lon,
 *                       N (1 - e2) sin lat),  N = a / sqrt(1 - e2 sin^2 lat)
 *     c = ecef(centre), p = ecef(corner), v = p - c, d = |v|
 *     t = c + ((factor * d + dist) / d) * v
 *     out_lon = atan2(t.y, t.x), out_lat = the geodetic latitude of t, its
 *     height dropped: th = atan2(a t.z, b q) with q = sqrt(t.x^2 + t.y^2),
 *     then THREE times  lat = atan2(t.z + e'2 b sin^3 th, q - e2 a cos^3 th),
 *     th = atan2(b sin lat, a cos lat)  (Bowring's iteration, a fixed count)
 * with three rules:
 *     A  a latitude >= pi/2 or <= -pi/2, of a corner or a centre, is the
 *        pole itself: ecef = (0, 0, +-b) whatever the longitude, so the two
 *        pole corners of a polar lat-lon cell come out as one point, bit for
 *        bit.  Such a corner crosses the pole when the expansion exceeds
 *        the cell.
 *     B  a corner with d == 0 (it IS the centre: the fixed point) is copied.
 *     C  slots k >= count[i] are copied.
 * One lane per slot; no LDS, no atomics on floating-point data: a pure
 * function of the inputs, and equal inputs give equal bits.
 *
 * status: two int32 on the device, the call's scratch.  The call WAITS for
 * its kernel on `stream`, reads them back and returns REMAP_ERR_ARG with a
 * message naming the bits below and the lowest offending cell when an input
 * is bad (out_lat / out_lon then hold copies at the offending slots).
 *
 *   REMAP_ERR_ARG   a NULL array, n_cells < 0 or > 2^31 - 1, width < 1, a
 *                   stride other than 0 or 1, more than 2^31 - 1 blocks of
 *                   256 slots; or an error bit
 *   n_cells == 0    REMAP_OK, nothing is launched (dist, factor and status
 *                   must still be given)
 * ---------------------------------------------------------------------------
 */
#define REMAP_EXPAND_ERR_COUNT 1  /* a count[i] outside [0, width]          */
#define REMAP_EXPAND_ERR_FINITE 2 /* NaN or Inf in a centre, a slot, dist or
                                     factor                                 */
#define REMAP_EXPAND_ERR_RADIUS 4 /* factor * d + dist <= 0 where d > 0     */

REMAP_API
int remap_expand_cells(int64_t n_cells, int32_t width,
                       const double *centre_lat, const double *centre_lon,
                       const double *corner_lat, const double *corner_lon,
                       const int32_t *count, const double *dist,
                       int32_t dist_stride, const double *factor,
                       int32_t factor_stride, double *out_lat,
                       double *out_lon, int32_t *status, void *stream);

/*
 * ---------------------------------------------------------------------------
 * What a complete mapping file says about its grids beyond the weights
 * (remap_geometry.hip): cell areas (area_a, area_b) and the fraction of every
 * source cell that takes part in the map (frac_a).
 *
 * remap_cell_areas: the area in steradians of every cell given in SCRIP
 * layout -- corner_lat / corner_lon (n_cells, width) row-major, radians, the
 * first count[i] slots of row i valid, 0 <= count[i] <= width -- as the
 * great-circle polygon of those corners.  Corners become unit vectors (a
 * latitude >= pi/2 or <= -pi/2 is the pole itself, whatever the longitude),
 * consecutive equal corners are dropped, the copies of corner 0 that close
 * the ring are dropped, and the area is
 *     | sum_k t(p_0, p_k, p_k+1) |,
 *     t(a, b, c) = 2 atan2(a . ((b - a) x (c - a)), 1 + a.b + b.c + c.a)
 * added in ascending k: the ring, the fan and the triangle of the overlap
 * calls' cell preparation (one device function serves both), so an MPAS
 * cell has the same bits here as in their a_area_out / b_area_out.  The sum
 * is signed, the absolute value is taken last: clockwise rings and concave
 * cells come out right.  Fewer than 3 corners left: 0.
 *
 * status: two int32 on the device, the call's scratch.  The call WAITS for
 * its kernel on `stream` and reads them back.
 *
 *   REMAP_ERR_ARG          a NULL array, n_cells < 0 or > 2^31 - 1, width <
 *                          1, or a count[i] outside [0, width] (the message
 *                          names the lowest such cell; its area_out is 0)
 *   REMAP_ERR_UNSUPPORTED  width > REMAP_CELL_AREAS_MAX_WIDTH
 *   n_cells == 0           REMAP_OK, nothing is launched (status must still
 *                          be given)
 * ---------------------------------------------------------------------------
 */
#define REMAP_CELL_AREAS_MAX_WIDTH 32

REMAP_API
int remap_cell_areas(int64_t n_cells, int32_t width, const double *corner_lat,
                     const double *corner_lon, const int32_t *count,
                     double *area_out, int32_t *status, void *stream);

/*
 * remap_column_fractions: out[j] (n_cols) = the sum of value[k] over the
 * entries with col[k] - index_base == j, added in ASCENDING k starting from
 * +0.0 -- numpy's bincount(col, weights=value) on the same entry order, bit
 * for bit -- then, for a column that has entries, divided by denom[j] when
 * denom is not NULL and replaced by 1 when clamp != 0 and it exceeds 1.  A
 * column without entries is +0.0.  With value = the overlap areas A (or
 * S * area_b[row]), denom = area_a and clamp = 1 this is ESMF's frac_a.
 *
 * No floating-point atomics: the entries are regrouped by column with a
 * stable radix sort (rocPRIM radix_sort_pairs, as remap_csr_from_coo; equal
 * keys keep their input order) and one lane adds one column up in that
 * order, so two calls give the same bytes.  A long column is added by its
 * one lane, serially.  Entries whose column is outside [0, n_cols) are left
 * out and counted in *bad_out (device, int64); nothing synchronises.
 *
 *   REMAP_ERR_ARG          a NULL array that is needed, a negative size
 *   REMAP_ERR_UNSUPPORTED  n_cols >= 2^31 or n_entries >= 2^32 - 1
 *   REMAP_ERR_WORKSPACE    workspace_bytes below
 *                          remap_column_fractions_workspace()'s answer
 */
REMAP_API
int remap_column_fractions_workspace(int64_t n_entries, size_t *bytes_out);

REMAP_API
int remap_column_fractions(int64_t n_entries, int64_t n_cols,
                           const int32_t *col, int32_t index_base,
                           const double *value, const double *denom,
                           int32_t clamp, double *out, int64_t *bad_out,
                           void *workspace, size_t workspace_bytes,
                           void *stream);

/*
 * ---------------------------------------------------------------------------
 * Second-order conservative maps (conserve2nd) from the first-order overlaps
 * ---------------------------------------------------------------------------
 * Everything on the unit sphere, cells great-circle polygons as in the
 * overlap calls.  The first moment M(P) = integral over P of r dA of a
 * polygon with corners p_0 .. p_n-1 (counter-clockwise, closed cyclically) is
 *     M = 1/2 sum_k theta_k n_k,   n_k = (p_k x p_k+1) / |p_k x p_k+1|,
 *     theta_k = atan2(|p_k x p_k+1|, p_k . p_k+1),
 * added in ascending k, p_k x p_k+1 evaluated as p_k x (p_k+1 - p_k); an
 * edge with p_k == p_k+1 adds nothing.  A source cell j has area A_j, moment
 * M_j, mean position M_j / A_j (NOT normalised) and centroid M_j / |M_j|.
 * The map's triples are (i, j, A_ij / A_i) for every first-order entry and,
 * where cell j has a gradient, (i, k, G_jk . d_ij) for k = j and j's edge
 * neighbours, d_ij = (M_ij - A_ij M_j / A_j) / A_i.  The G of a cell sum to
 * 0, so the rows keep their first-order sums; sum_i M_ij = M_j for a fully
 * covered source cell j, so sum_i A_i S_ik = A_k for every source cell k that
 * is fully covered together with its edge neighbours.  This is ESMF's
 * conserve2nd in structure, not in bytes.  All calls: fp64, on the caller's
 * stream, no floating-point atomics (two calls give the same bytes).
 *
 * remap_cell_moments: moment_out (n_cells x 3) of cells in SCRIP layout, the
 * arguments, the ring (consecutive equal corners and closing copies dropped)
 * and the errors of remap_cell_areas.  A clockwise ring (its moment points
 * away from the sum of its corners) is negated at the end; fewer than 3
 * distinct corners: 0.  status: two int32 on the device; the call WAITS.
 *
 * remap_overlap_moments: moment_out (n_entries x 3), M_ij of source cell
 * src[e] n destination cell dst[e] (0-based, as the overlap calls return
 * them), both sides in SCRIP layout (width <= REMAP_OVERLAP_MAX_EDGES each,
 * REMAP_ERR_UNSUPPORTED otherwise).  The source cell is clipped by the
 * destination cell's edges in the gnomonic plane of the source cell's centre
 * (the normalised sum of its corners): the ring loading and the edge clip of
 * remap_overlap_meshes; the clipped corners are lifted back to unit vectors.
 * A clip that leaves fewer than 3 corners gives area[e] * src_moment[j] /
 * src_area[j] (no correction).  Destination cells must be convex
 * (REMAP_OVERLAP_ERR_CONVEX) and every corner of a pair within acos(0.1) of
 * the source cell's centre (REMAP_OVERLAP_ERR_HEMISPHERE): both
 * REMAP_ERR_UNSUPPORTED.  An entry outside its side, a count outside
 * [0, width]: REMAP_ERR_ARG.  workspace: remap_overlap_moments_workspace()
 * bytes (the prepared rings).  status: two int32 on the device; the call
 * WAITS twice (the source's counts, then everything else).
 *
 * remap_gradient_stencils: nbr (n_cells x width, -1 = no cell across edge
 * (corner t, corner t + 1)), count = nEdgesOnCell, centroid (n_cells x 3,
 * unit).  A cell has a gradient (has_out = 1) when count >= 3, every edge has
 * a neighbour and the polygon N of the neighbours' centroids, in edge order,
 * has an area A_N != 0.  With nu_t / theta_t the unit normal / the arc
 * between neighbours t and t + 1 (cyclic) and e_t = -1/2 theta_t nu_t / A_N
 * (A_N SIGNED: a clockwise N gives what its reversal gives), coef_out
 * (n_cells x (width + 1) x 3) holds at slot 1 + t  e_t-1 + e_t  and at slot 0
 * -2 sum_t e_t, each made tangential: G - (G . c_j) c_j.  A cell without a
 * gradient has all 0.  width <= REMAP_OVERLAP_MAX_EDGES.  status as above;
 * the call WAITS.  REMAP_ERR_ARG: a count outside [0, width], a neighbour >=
 * n_cells.
 *
 * remap_conserve2nd_sizes: *capacity_out = the number of triples (1 per
 * entry, + 1 + count[j] where has[j]), read back (the call WAITS), and the
 * workspace bytes of the assembly.  counters: two int64 on the device.
 *
 * remap_conserve2nd_assemble: triples in emission order (entry order; the
 * first-order term, the cell itself, the neighbours in edge order), the dot
 * product as (gx*dx + gy*dy) + gz*dz; keys row << 32 | col with the emission
 * position as value, stable radix sort, equal keys added in emission order,
 * zero sums kept.  row_out / col_out (0-based) / s_out hold `capacity`
 * slots, the first *n_out (host; the one read-back, the call WAITS) are the
 * map sorted by (row, col), unique.  REMAP_ERR_ARG: an index outside its
 * side, a capacity that is not remap_conserve2nd_sizes' for these arrays.
 * ---------------------------------------------------------------------------
 */
REMAP_API
int remap_cell_moments(int64_t n_cells, int32_t width,
                       const double *corner_lat, const double *corner_lon,
                       const int32_t *count, double *moment_out,
                       int32_t *status, void *stream);

REMAP_API
int remap_overlap_moments_workspace(int64_t n_src, int32_t width_src,
                                    int64_t n_dst, int32_t width_dst,
                                    size_t *bytes_out);

REMAP_API
int remap_overlap_moments(int64_t n_entries, const int32_t *dst,
                          const int32_t *src, const double *area,
                          int64_t n_src, int32_t width_src,
                          const double *src_lat, const double *src_lon,
                          const int32_t *src_count, const double *src_area,
                          const double *src_moment, int64_t n_dst,
                          int32_t width_dst, const double *dst_lat,
                          const double *dst_lon, const int32_t *dst_count,
                          double *moment_out, int32_t *status,
                          void *workspace, size_t workspace_bytes,
                          void *stream);

REMAP_API
int remap_gradient_stencils(int64_t n_cells, int32_t width,
                            const int32_t *nbr, const int32_t *count,
                            const double *centroid, double *coef_out,
                            int32_t *has_out, int32_t *status, void *stream);

REMAP_API
int remap_conserve2nd_sizes(int64_t n_entries, const int32_t *src,
                            int64_t n_src, int32_t width,
                            const int32_t *count, const int32_t *has,
                            int64_t *counters, int64_t *capacity_out,
                            size_t *workspace_bytes_out, void *stream);

REMAP_API
int remap_conserve2nd_assemble(int64_t n_entries, const int32_t *dst,
                               const int32_t *src, const double *area,
                               const double *moment, int64_t n_src,
                               int32_t width, const int32_t *nbr,
                               const int32_t *count, const double *coef,
                               const int32_t *has, const double *src_area,
                               const double *src_moment, int64_t n_dst,
                               const double *dst_area, int64_t capacity,
                               void *workspace, size_t workspace_bytes,
                               int32_t *row_out, int32_t *col_out,
                               double *s_out, int64_t *counters,
                               int64_t *n_out, void *stream);

/*
 * ---------------------------------------------------------------------------
 * Patch-recovery maps (patch) on the triangles remap_locate searches
 * ---------------------------------------------------------------------------
 * ESMF's patch interpolation in structure, not in bytes: a least-squares
 * quadratic per node over its one-ring, and per destination point the blend
 * of its triangle's three quadratics by the located weights, written as a
 * map row.  xyz (n_nodes x 3, unit), tri (n_tri x 3 node ids) and points
 * (n_pts x 3, unit) as remap_locate takes them, found / w as it returns them.
 * Additions of ABI 31: no existing call changes.
 *
 * Rings.  ring[v] (REMAP_PATCH_MAX_RING wide) holds the distinct nodes that
 * share a triangle with v, v itself left out, ascending, padded with -1;
 * count[v] is their true number, of which the lowest REMAP_PATCH_MAX_RING are
 * kept.  (The six directed pairs (a, b) of every triangle keyed a << 32 | b,
 * rocPRIM's radix sort, the heads of the runs ranked by a scan and segmented
 * per node.)
 *
 * Fits.  The members of node v are v, then ring[v].  The frame at c = xyz[v]:
 * ref = z if |c_z| < 0.9, else x; e1 = normalize(ref x c); e2 = c x e1.
 * Member r has t = r . c, x = (r . e1) / t, y = (r . e2) / t; h = the largest
 * sqrt(x^2 + y^2) of the members; phi = (1, x/h, y/h, (x/h)^2, (x/h)(y/h),
 * (y/h)^2); N = sum phi phi^T, the members added in order.  v HAS A PATCH
 * when it has at least 6 members, count[v] <= REMAP_PATCH_MAX_RING (and is
 * the number of ring slots filled), every member has t > 0.5, everything is
 * finite and the unpivoted Cholesky N = L L^T (row by row) has every pivot
 * d_k > 1e-2 N_kk.  fit[v] (REMAP_PATCH_FIT_WIDTH = 22 doubles) is h followed
 * by the upper triangle of N^-1 = M^T M, M = L^-1, row-major; without a patch
 * fit[v] = 0 and has[v] = 0.  (The pivot share was 1e-8 when ABI 31 came; it
 * admitted fits singular to eight digits on the duals of edge and vertex
 * meshes.  No signature or layout changed, so the ABI number stays; no node
 * of a cell mesh changes, their smallest share is 0.19.)
 *
 * Rows.  A point p with found[p] = f >= 0 in triangle (v0, v1, v2) gets the
 * bilinear row (v_t, w[p][t]) bit for bit when one of the three nodes has no
 * patch or p . xyz[v_t] <= 0.5 for some t.  Otherwise, for t = 0, 1, 2: with
 * phi_p the basis at p's scaled coordinates in v_t's frame and g = N^-1
 * phi_p, member k of v_t receives w[p][t] * (phi_k . g).  Triples with the
 * same column are added in emission order (t ascending, members in order)
 * and the row is written sorted by column, zero sums kept.  Because every
 * member list is ascending once v_t is put in its place, the row is ONE
 * three-way merge of the lists: no per-lane list, no sort.  found[p] = -1:
 * no row.
 *
 * remap_node_rings: ring_out (n_nodes x 16) and count_out (n_nodes) from tri.
 * workspace: remap_node_rings_workspace() bytes.  status: one int32 on the
 * device; the call WAITS (REMAP_ERR_ARG: a triangle names a node outside
 * [0, n_nodes)).  n_tri < 2^32 / 6.
 *
 * remap_patch_fits: fit_out (n_nodes x 22) and has_out (n_nodes), one lane
 * per node.  status as above; the call WAITS (REMAP_ERR_ARG: a ring entry
 * outside [-1, n_nodes)).
 *
 * remap_patch_sizes: offsets_out (n_pts + 1 int64 on the device): the
 * exclusive scan of every row's number of distinct columns, offsets_out[n_pts]
 * = *total_out (host; the one read-back, the call WAITS).  workspace:
 * remap_patch_sizes_workspace() bytes.
 *
 * remap_patch_rows: row p into row_out / col_out (0-based) / s_out at
 * [offsets[p], offsets[p + 1]); capacity = the slots of the three arrays =
 * offsets[n_pts].  The output is sorted by (row, col), unique.  Nothing is
 * written outside a row's own slots.  status as above; the call WAITS.
 * REMAP_ERR_ARG: a node or triangle id outside its side, offsets that are not
 * remap_patch_sizes' for these arrays.
 *
 * All calls: fp64, on the caller's stream, no floating-point atomics (two
 * calls give the same bytes).
 * ---------------------------------------------------------------------------
 */
#define REMAP_PATCH_MAX_RING 16
#define REMAP_PATCH_FIT_WIDTH 22

REMAP_API
int remap_node_rings_workspace(int64_t n_tri, int64_t n_nodes,
                               size_t *bytes_out);

REMAP_API
int remap_node_rings(int64_t n_tri, const int32_t *tri, int64_t n_nodes,
                     int32_t *ring_out, int32_t *count_out, int32_t *status,
                     void *workspace, size_t workspace_bytes, void *stream);

REMAP_API
int remap_patch_fits(int64_t n_nodes, const double *xyz, const int32_t *ring,
                     const int32_t *count, double *fit_out, int32_t *has_out,
                     int32_t *status, void *stream);

REMAP_API
int remap_patch_sizes_workspace(int64_t n_pts, size_t *bytes_out);

REMAP_API
int remap_patch_sizes(int64_t n_nodes, const double *xyz, int64_t n_tri,
                      const int32_t *tri, const int32_t *ring,
                      const int32_t *count, const int32_t *has, int64_t n_pts,
                      const int32_t *found, const double *points,
                      int64_t *offsets_out, int64_t *total_out,
                      int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream);

REMAP_API
int remap_patch_rows(int64_t n_nodes, const double *xyz, int64_t n_tri,
                     const int32_t *tri, const int32_t *ring,
                     const int32_t *count, const double *fit,
                     const int32_t *has, int64_t n_pts, const int32_t *found,
                     const double *w, const double *points,
                     const int64_t *offsets, int64_t capacity,
                     int32_t *row_out, int32_t *col_out, double *s_out,
                     int32_t *status, void *stream);

/* ---------------------------------------------------------------------------
 * Local-bounds limiter (csrc/remap_limit.hip; DESIGN.md section 20;
 * pyremap_amd.limiter is the same statement in numpy).
 *
 * A map with signed weights (conserve2nd, patch, a signed map read from a
 * file) overshoots at fronts.  This pass runs AFTER an apply launch, on the
 * same stream and over the same strided layouts, and clamps every
 * destination value to the bounds of the source values of its own row.  It
 * re-gathers them from the CSR (rowptr, col); the weights are not read: every
 * stored entry counts, whatever the sign or size of its weight.
 *
 * For destination element (i, b, k), row_begin <= i < row_end, the row's
 * entries are walked in CSR order with x = (double)X[cell(col), b, k]:
 *   a NaN x is skipped (+-inf are values like any other);
 *   the first x that is no NaN sets lo = hi = x; after it
 *   if (x < lo) lo = x; if (x > hi) hi = x;  -- strict: the first one seen
 *   wins a tie, so -0.0 against +0.0 is decided by CSR order;
 *   a row without an entry, or without a value that is no NaN: y stays as it
 *   is and lo = hi = y; otherwise y = y < lo ? lo : (y > hi ? hi : y) (a NaN
 *   y stays NaN).
 * y is written back in place, lo / hi where those pointers are given.
 * Elements of rows outside [row_begin, row_end) are not written.  Nothing
 * rounds: comparisons and copies only, the result is defined to the bit.
 *
 * X and Y are addressed as in remap_apply_args (x_src_fold included); lo and
 * hi like Y.  Asynchronous on `stream`; nothing is allocated, freed or
 * synchronised.  REMAP_ERR_ARG: a NULL array that is needed, a negative
 * stride or size, a row range outside [0, A.n_rows], an x_dtype that is no
 * REMAP_DTYPE_*, an x_src_fold that does not divide A.n_cols, more elements
 * than one launch serves.
 * ---------------------------------------------------------------------------
 */
typedef struct remap_limit_args {
    remap_csr A;            /* rowptr and col are read; val is not           */
    int64_t row_begin;      /* rows [row_begin, row_end) of A are limited;   */
    int64_t row_end;        /* Y / lo / hi are indexed by row                */
    const void *X;          /* (device) the source field the apply read      */
    int32_t x_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t x_row_stride;
    int64_t x_batch_stride;
    int64_t x_src_fold;     /* as in remap_apply_args (0: one stride)        */
    int64_t x_outer_stride;
    double *Y;              /* (device) what the apply left, limited in place */
    int64_t y_row_stride;
    int64_t y_batch_stride;
    int64_t n_batch;
    int64_t k_inner;
    double *lo;             /* (device) optional, addressed like Y           */
    double *hi;             /* (device) optional, addressed like Y           */
} remap_limit_args;

REMAP_API int remap_limit_rows(const struct remap_limit_args *args,
                               void *stream);

/* ---------------------------------------------------------------------------
 * Sub-gridscale fraction weighting (csrc/remap_sgs.hip; DESIGN.md section 21;
 * pyremap_amd.sgs is the same statement in numpy).
 *
 * A field that is a mean over a FRACTION of every source cell (ice thickness
 * over the ice-covered part, NCO's `ncremap --sgs_frc`) is multiplied by the
 * fraction before the map and divided by the remapped fraction after it, in
 * one launch: X is read once, as REMAP_MODE_MASKED reads it, plus a fraction
 * F that is usually k_inner times smaller.
 *
 * For destination element (i, b, k), the entries j of row i are walked in CSR
 * order.  Three float64 accumulators start at +0.0.
 *
 *   x = (double) X[cell(col_j), b, k]
 *   f = (double) F[cell(col_j), b', k']     (b', k': b, k or 0 where F is broadcast)
 *   the entry counts iff x is no NaN and f is no NaN      (+-inf, 0 and negative f are values)
 *   counts:  t = f * x;   num += S_j * t;   den += S_j * f;   valid += S_j
 *            (every product rounded, every sum rounded: no FMA contraction)
 *   y = (valid > threshold && den > 0) ? num / den : NaN
 *
 * Every NaN written is the quiet NaN 0x7ff8000000000000, also where num / den
 * is itself a NaN (inf / inf): the bits of Y are defined.
 *
 * This is the reference's masked branch (remap_numpy.py:262-266) with in_mask
 * replaced by a real-valued fraction.  With F == 1 everywhere the result is
 * byte for byte REMAP_MODE_MASKED at the same threshold; scaling F by a power
 * of two (without overflow or denormals) keeps the bytes of Y.  A map with
 * signed weights (conserve2nd, patch) can give den <= 0: y is NaN there.
 *
 * X and Y are addressed as in remap_limit_args (x_src_fold included).  F is
 * addressed like X with strides of its own:
 *   F[b * f_batch_stride + cell(a) + k * f_inner_stride],
 *   cell(a) = a * f_row_stride, or with x_src_fold != 0
 *   (a / x_src_fold) * f_outer_stride + (a % x_src_fold) * f_row_stride.
 * f_batch_stride == 0 broadcasts over the batches, f_inner_stride (0 or 1)
 * == 0 over the inner index: a (Time, nCells) fraction for (Time, nCells,
 * nCategories) fields.
 *
 * Elements of rows outside [row_begin, row_end) are not written.
 * Asynchronous on `stream`; nothing is allocated, freed or synchronised.
 * REMAP_ERR_ARG: a NULL array that is needed, a negative stride or size, an
 * f_inner_stride that is neither 0 nor 1, a row range outside [0, A.n_rows],
 * an x_dtype or f_dtype that is no REMAP_DTYPE_*, an x_src_fold that does not
 * divide A.n_cols, more elements than one launch serves.
 * ---------------------------------------------------------------------------
 */
typedef struct remap_sgs_args {
    remap_csr A;            /* rowptr, col and val are all read              */
    int64_t row_begin;      /* rows [row_begin, row_end) of A are computed;  */
    int64_t row_end;        /* Y is indexed by row                           */
    const void *X;          /* (device) source field                         */
    int32_t x_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t x_row_stride;
    int64_t x_batch_stride;
    int64_t x_src_fold;     /* as in remap_apply_args (0: one stride)        */
    int64_t x_outer_stride;
    const void *F;          /* (device) sub-gridscale fraction               */
    int32_t f_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t f_row_stride;
    int64_t f_batch_stride; /* 0: the same fraction in every batch           */
    int64_t f_inner_stride; /* 1, or 0: the same fraction for every k        */
    int64_t f_outer_stride; /* with x_src_fold != 0, as x_outer_stride       */
    double *Y;              /* (device) destination field, float64           */
    int64_t y_row_stride;
    int64_t y_batch_stride;
    int64_t n_batch;
    int64_t k_inner;
    double threshold;       /* of `valid`, as REMAP_MODE_MASKED has it       */
} remap_sgs_args;

REMAP_API int remap_apply_sgs(const struct remap_sgs_args *args,
                              void *stream);

/* ---------------------------------------------------------------------------
 * Vector fields (csrc/remap_vector.hip; DESIGN.md section 22;
 * pyremap_amd.vector is the same statement in numpy).
 *
 * The zonal and meridional components of a velocity, a wind stress or an ice
 * drift are no scalars: the east and north directions of the source cells of
 * one row's stencil differ from those at the destination point, near a pole
 * by tens of degrees.  This launch rotates every source vector to Cartesian
 * (x, y, z), sums the three components with the row's weights and projects
 * the sum on the destination cell's east and north, in one pass: U and V are
 * read once each, YU and YV written once each.
 *
 * Inputs: two source fields U (eastward) and V (northward) of one shape,
 * dtype and layout, a source basis BA (n_a, 5) fp64 with rows
 * (ex, ey, nx, ny, nz) and a destination basis BB (n_b, 5) fp64 of the same
 * kind, with
 *   ex = -sin(lon), ey = cos(lon),
 *   nx = -sin(lat) cos(lon), ny = -sin(lat) sin(lon), nz = cos(lat)
 * (the z-component of east is 0).  The bases are made on the host from the
 * centres in the mapping file: device trigonometry never enters the bits.
 *
 * For destination element (i, b, k) the entries j of row i are walked in CSR
 * order.  Four float64 accumulators start at +0.0.
 *
 *   u = (double) U[cell(col_j), b, k];  v = (double) V[cell(col_j), b, k]
 *   the entry counts iff neither is a NaN; then, with the basis row of cell col_j:
 *     px = u*ex + v*nx;   py = u*ey + v*ny;   pz = v*nz      (each product rounded, then the sum)
 *     cx += S_j*px;  cy += S_j*py;  cz += S_j*pz;  valid += S_j
 *   with the basis row (Ex, Ey, Nx, Ny, Nz) of destination cell i:
 *     tu = cx*Ex + cy*Ey;      tv = (cx*Nx + cy*Ny) + cz*Nz
 *     valid > threshold:  yu = tu / valid,  yv = tv / valid
 *     otherwise:          both NaN
 *
 * No FMA contraction; an entry that does not count is skipped, not added as
 * a zero.  Every NaN written is the quiet NaN 0x7ff8000000000000, also where
 * a quotient is itself a NaN.  This is the reference's masked branch
 * (remap_numpy.py:262-266) with the mask the union of the two components'.
 * With every basis row (1, 0, 0, 1, 0) and finite fields YU and YV are byte
 * for byte REMAP_MODE_MASKED of U and of V under that union.
 *
 * U and V are addressed as X is in remap_sgs_args, with ONE dtype and one
 * set of strides (x_src_fold included); YU and YV like Y, with one set of
 * strides.  BA and BB are dense, row stride 5.
 *
 * Elements of rows outside [row_begin, row_end) are not written.
 * Asynchronous on `stream`; nothing is allocated, freed or synchronised.
 * REMAP_ERR_ARG: a NULL array that is needed, a negative stride or size, a
 * row range outside [0, A.n_rows], an x_dtype that is no REMAP_DTYPE_*, an
 * x_src_fold that does not divide A.n_cols, more elements than one launch
 * serves.
 * ---------------------------------------------------------------------------
 */
typedef struct remap_vector_args {
    remap_csr A;            /* rowptr, col and val are all read              */
    int64_t row_begin;      /* rows [row_begin, row_end) of A are computed;  */
    int64_t row_end;        /* YU, YV and BB are indexed by row              */
    const void *U;          /* (device) eastward source component            */
    const void *V;          /* (device) northward source component           */
    int32_t x_dtype;        /* REMAP_DTYPE_*, of U and of V                  */
    int64_t x_row_stride;   /* of U and of V                                 */
    int64_t x_batch_stride;
    int64_t x_src_fold;     /* as in remap_apply_args (0: one stride)        */
    int64_t x_outer_stride;
    const double *BA;       /* (device) (A.n_cols, 5) source basis           */
    const double *BB;       /* (device) (A.n_rows, 5) destination basis      */
    double *YU;             /* (device) eastward destination component       */
    double *YV;             /* (device) northward destination component      */
    int64_t y_row_stride;   /* of YU and of YV                               */
    int64_t y_batch_stride;
    int64_t n_batch;
    int64_t k_inner;
    double threshold;       /* of `valid`, as REMAP_MODE_MASKED has it       */
} remap_vector_args;

REMAP_API int remap_apply_vector(const struct remap_vector_args *args,
                                 void *stream);

/* ---------------------------------------------------------------------------
 * Columns interpolated to target levels inside the apply: depth slices
 * (csrc/remap_levels.hip; pyremap_amd.levels is the
 * same statement in numpy).
 *
 * Level k of an MPAS-Ocean (Time, nCells, nVertLevels) field sits at another
 * depth in every cell (zMid), and its columns end at another bottom in every
 * cell.  This launch interpolates, for every entry of a row, the source
 * column to the target level first and lets the value enter the masked,
 * renormalised sum then: the field at a depth, in one pass, without the
 * (.., nCells, L) intermediate.  An entry whose column does not reach the
 * level is skipped exactly as a NaN is.
 *
 * Inputs: the source field X[cell, b, k], k < n_levels, fp32 or fp64; the
 * level coordinate Z[cell, b', k], fp32 or fp64 independently of X; the
 * targets T[l], l < k_inner, fp64 on the device, in any order, duplicates
 * allowed.  Every float32 widens to double first.
 *
 * For destination element (i, b, l), the entries j of row i are walked in CSR
 * order.  Two float64 accumulators start at +0.0.
 *
 *   t = T[l];   z_k = (double) Z[cell(col_j), b', k];   x_k = (double) X[cell(col_j), b, k]
 *   walk k = 0 .. n_levels-1 in ascending order and stop at the first hit:
 *     node hit:      t == z_k:   v = x_k      (x_{k+1} is not looked at)
 *     interior hit:  k+1 < n_levels and (z_k < t && t < z_{k+1}  or  z_k > t && t > z_{k+1}):
 *                    w = (t - z_k) / (z_{k+1} - z_k);   v = x_k + w * (x_{k+1} - x_k)
 *     no hit:        the column has no value at this level
 *   the entry counts iff its column has a hit and v is no NaN
 *   counts:  num += S_j * v;   valid += S_j      (every operation rounded on its own: no FMA contraction)
 *   y = (valid > threshold) ? num / valid : NaN
 *
 * Comparisons with a NaN are false, so a NaN in Z never brackets anything.
 * Columns may rise or fall; nothing assumes that they are monotone; nothing
 * is extrapolated above the first or below the last valid level.  Every NaN
 * written is the quiet NaN 0x7ff8000000000000, also where num / valid is
 * itself a NaN.  The result is byte for byte REMAP_MODE_MASKED, at the same
 * threshold, of the array of column values with NaN where an entry does not
 * count.  With one strictly monotone Z shared by all cells and T = Z[ks] it
 * is the masked apply of X[..., ks].
 *
 * X and Y are addressed as in remap_sgs_args (x_src_fold included), with
 * n_levels the inner extent of X (stride 1) and k_inner = L the inner extent
 * of Y.  Z is addressed like X with strides of its own:
 *   Z[b * z_batch_stride + cell(a) + k],
 *   cell(a) = a * z_row_stride, or with x_src_fold != 0
 *   (a / x_src_fold) * z_outer_stride + (a % x_src_fold) * z_row_stride.
 * z_row_stride == 0 (with z_outer_stride == 0) is one coordinate for all
 * cells, z_batch_stride == 0 a time-invariant coordinate.
 *
 * Elements of rows outside [row_begin, row_end) are not written.
 * Asynchronous on `stream`; nothing is allocated, freed or synchronised.
 * REMAP_ERR_ARG: what remap_apply_sgs refuses (a NULL array that is needed,
 * a negative stride or size, a row range outside [0, A.n_rows], an x_dtype
 * that is no REMAP_DTYPE_*, an x_src_fold that does not divide A.n_cols, more
 * elements than one launch serves), n_levels < 1, a NULL Z or T, a negative Z
 * stride, a z_dtype that is no REMAP_DTYPE_*.
 * ---------------------------------------------------------------------------
 */
typedef struct remap_levels_args {
    remap_csr A;            /* rowptr, col and val are all read              */
    int64_t row_begin;      /* rows [row_begin, row_end) of A are computed;  */
    int64_t row_end;        /* Y is indexed by row                           */
    const void *X;          /* (device) source field, n_levels per column    */
    int32_t x_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t x_row_stride;
    int64_t x_batch_stride;
    int64_t x_src_fold;     /* as in remap_apply_args (0: one stride)        */
    int64_t x_outer_stride;
    int64_t n_levels;       /* inner extent of X and of Z, stride 1          */
    const void *Z;          /* (device) level coordinate                     */
    int32_t z_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t z_row_stride;   /* 0: one coordinate for all cells               */
    int64_t z_batch_stride; /* 0: the same coordinate in every batch         */
    int64_t z_outer_stride; /* with x_src_fold != 0, as x_outer_stride       */
    const double *T;        /* (device) k_inner target levels                */
    double *Y;              /* (device) destination field, float64           */
    int64_t y_row_stride;
    int64_t y_batch_stride;
    int64_t n_batch;
    int64_t k_inner;        /* L: the inner extent of Y                      */
    double threshold;       /* of `valid`, as REMAP_MODE_MASKED has it       */
} remap_levels_args;

REMAP_API int remap_apply_levels(const struct remap_levels_args *args,
                                 void *stream);

/* ---------------------------------------------------------------------------
 * Columns averaged or integrated over depth ranges inside the apply: layer
 * means, heat content (csrc/remap_layers.hip; DESIGN.md section 24;
 * pyremap_amd.layers is the same statement in numpy).
 *
 * remap_apply_levels gives the field AT a depth; this launch gives the field
 * OVER a depth range.  Every entry of a row first reduces its source column
 * over the range -- the overlap of every layer with the range weighs the
 * layer's value; a range may cut through a layer, a column may end inside
 * the range or above it -- and enters the masked, renormalised sum then: one
 * pass, without the (.., nCells, R) intermediate.
 *
 * Inputs: the source field X[cell, b, k], k < n_levels, fp32 or fp64; the
 * layer thicknesses H[cell, b', k], fp32 or fp64 independently of X; the
 * ranges bounds[2 r] = A_r, bounds[2 r + 1] = B_r, r < k_inner, fp64 on the
 * device, in any order, duplicates allowed.  Every float32 widens to double
 * first.  Depths are positive downward, measured from the top of each
 * column's first layer.
 *
 * For destination element (i, b, r), with range [A, B] = [A_r, B_r], the
 * entries j of row i are walked in CSR order.  Two float64 accumulators num
 * and valid start at +0.0.  For each entry the source column c = cell(col_j)
 * is walked k = 0 .. n_levels-1 ascending, from d = v = t = +0.0:
 *
 *   h = (double) H[c, b', k]
 *   if !(h > 0): the layer is not there (NaN, zero, negative): skip it, d stays
 *   top = d;  d = d + h
 *   lo = top > A ? top : A;   hi = d < B ? d : B
 *   if hi > lo:  o = hi - lo;  x = (double) X[c, b, k]
 *                if x == x:  p = o * x;  v = v + p;  t = t + o
 *   (the walk may stop once top >= B: nothing further can overlap)
 *   the entry counts iff t > 0 and q is no NaN:  q = v / t (mean),  q = v (integral)
 *   counts:  p = S_j * q;  num = num + p;  valid = valid + S_j      (every operation rounded on its own: no FMA contraction)
 *   y = (valid > threshold) ? num / valid : NaN
 *
 * Comparisons with a NaN are false: a NaN bound gives an empty range, B =
 * +inf means "to the bottom".  A layer whose value is a NaN leaves both sums
 * of its column; a column that ends above A is skipped exactly as a NaN is
 * (the bathymetry mask needs no input of its own); a column that ends inside
 * the range contributes what it has.  Every NaN written is the quiet NaN
 * 0x7ff8000000000000, also where num / valid is itself a NaN.  The result is
 * byte for byte REMAP_MODE_MASKED, at the same threshold, of the array of
 * column values q with NaN where an entry does not count.
 *
 * X and Y are addressed as in remap_levels_args (x_src_fold included), with
 * n_levels the inner extent of X (stride 1) and k_inner = R the inner extent
 * of Y.  H is addressed like X with strides of its own:
 *   H[b * h_batch_stride + cell(a) + k],
 *   cell(a) = a * h_row_stride, or with x_src_fold != 0
 *   (a / x_src_fold) * h_outer_stride + (a % x_src_fold) * h_row_stride.
 * h_row_stride == 0 (with h_outer_stride == 0) is one thickness column for
 * all cells, h_batch_stride == 0 a time-invariant thickness.
 *
 * Elements of rows outside [row_begin, row_end) are not written.
 * Asynchronous on `stream`; nothing is allocated, freed or synchronised.
 * REMAP_ERR_ARG: what remap_apply_levels refuses of the members the two
 * share, n_levels < 1, a NULL H or bounds, a negative H stride, an h_dtype
 * that is no REMAP_DTYPE_*, a reduce that is no REMAP_REDUCE_*.
 * ---------------------------------------------------------------------------
 */
#define REMAP_REDUCE_MEAN 0      /* q = v / t: the thickness-weighted mean  */
#define REMAP_REDUCE_INTEGRAL 1  /* q = v: the integral over the range      */

typedef struct remap_layers_args {
    remap_csr A;            /* rowptr, col and val are all read              */
    int64_t row_begin;      /* rows [row_begin, row_end) of A are computed;  */
    int64_t row_end;        /* Y is indexed by row                           */
    const void *X;          /* (device) source field, n_levels per column    */
    int32_t x_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t x_row_stride;
    int64_t x_batch_stride;
    int64_t x_src_fold;     /* as in remap_apply_args (0: one stride)        */
    int64_t x_outer_stride;
    int64_t n_levels;       /* inner extent of X and of H, stride 1          */
    const void *H;          /* (device) layer thicknesses                    */
    int32_t h_dtype;        /* REMAP_DTYPE_*                                 */
    int64_t h_row_stride;   /* 0: one thickness column for all cells         */
    int64_t h_batch_stride; /* 0: the same thicknesses in every batch        */
    int64_t h_outer_stride; /* with x_src_fold != 0, as x_outer_stride       */
    const double *bounds;   /* (device) 2 * k_inner doubles: A_0, B_0, A_1.. */
    double *Y;              /* (device) destination field, float64           */
    int64_t y_row_stride;
    int64_t y_batch_stride;
    int64_t n_batch;
    int64_t k_inner;        /* R: the inner extent of Y                      */
    double threshold;       /* of `valid`, as REMAP_MODE_MASKED has it       */
    int32_t reduce;         /* REMAP_REDUCE_*                                */
} remap_layers_args;

REMAP_API int remap_apply_layers(const struct remap_layers_args *args,
                                 void *stream);

#ifdef __cplusplus
}
#endif

#endif /* REMAP_HIP_H */
