/* include/edt_hip.h -- C ABI of the MI355X-native multi-label anisotropic EDT.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The entry
 * points below are exactly what the reference's FFI for this path binds
 * (`cdef extern from "edt.hpp" namespace "pyedt"`, /root/reference/src/edt.pyx:62-113),
 * with the template parameter T replaced by a run-time `dtype` code.  INTEGRATION.md shows
 * the reference-side stubs (Cython / C++ header) a maintainer would add.
 *
 * Conventions (identical to the reference, src/edt.hpp:411-484):
 *   - x is the fastest axis: idx = x + sx * (y + sy * z);
 *   - label 0 is background; any change of label is a boundary;
 *   - wx, wy, wz are the physical voxel sizes (anisotropy) as fp32; every size of an axis the call uses
 *     must be finite and non-zero, wx positive, or the call fails with EDT_ERR_BAD_ARG before any device
 *     work.  A negative wy / wz is taken as |w|: along y and z a size enters only as its square
 *     (src/edt.hpp:181, :258), which is what the reference computes with it.  (Stated deviation for the
 *     rest: the reference does not validate -- a negative wx makes its pass 1 cross label boundaries,
 *     src/edt.hpp:107-109, NaN / inf / 0 give NaN or all-zero fields);
 *   - black_border != 0 treats the outside of the volume as background;
 *   - output is fp32, squared distances unless the entry point says otherwise;
 *     with black_border == 0 voxels that see no boundary are +INF.
 *   - `parallel` is accepted for signature compatibility and ignored (the GPU grid
 *     replaces the reference's ThreadPool, src/threadpool.h:46-140).
 *   - labels are integers of 1/2/4/8 bytes (signed ones read as their unsigned bit patterns), IEEE binary32 /
 *     binary64 or bool bytes: the dtype codes below.  (Stated deviation: the reference's templates also take
 *     long double; cpp/edt.hpp refuses it, and every other width, at compile time.)
 *
 * Every function returns EDT_OK (0) or a negative error code and never throws;
 * edt_hip_last_error() describes the last failure on the calling thread.  There is NO
 * CPU fallback inside this library: without a usable gfx950 device every compute entry
 * point fails with EDT_ERR_NO_DEVICE.
 */
#ifndef EDT_HIP_H
#define EDT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* label element types (the seven instantiations of src/edt.pyx:670-732) */
enum {
  EDT_U8 = 0,
  EDT_U16 = 1,
  EDT_U32 = 2,
  EDT_U64 = 3,
  EDT_F32 = 4,
  EDT_F64 = 5,
  EDT_BOOL = 6 /* one byte per voxel, any non-zero byte is foreground */
};

enum {
  EDT_OK = 0,
  EDT_ERR_NO_DEVICE = -1,
  EDT_ERR_BAD_ARG = -2,
  EDT_ERR_HIP = -3,
  EDT_ERR_UNSUPPORTED = -4,
  EDT_ERR_NOMEM = -5
};

/* flags for the device-resident entry points */
enum {
  EDT_FLAG_BLACK_BORDER = 1, /* treat the outside of the volume as background          */
  EDT_FLAG_SQRT = 2,         /* return distances instead of squared distances          */
  EDT_FLAG_FORCE_GENERIC = 4, /* use the size-agnostic fallback kernels (test hook)     */
  EDT_FLAG_BATCH_2D = 8,     /* edt_hip_edtsq_device with ndim = 3: the volume is a STACK of sz independent
                                2-D images (sx x sy each) -- x and y passes only, one launch for all images */
  EDT_FLAG_BINARY_YZ = 32,   /* the reference's *binary* route for a multi-valued label type (pyedt::_binary_edt{2,3}dsq<T>,
                                src/edt.hpp:487-576, :681-755): labels split runs in pass X only; passes Y and Z treat every
                                column as one envelope from its first non-zero value on, background voxels as height-0
                                sites.  Identical to the ordinary transform on 0/1 input. */
  EDT_FLAG_SIGNED = 64,      /* edt_hip_edtsq_device: the SIGNED transform -- sdf / sdfsq of the reference's Python layer
                                (src/edt.pyx:121-202: edt(x) - edt(x == 0)) as ONE transform: label 0 is measured like every
                                other label and its voxels come out negated.  Bit-identical to the two-transform definition
                                (the two fields have disjoint supports, and a voxel's value depends only on the voxels of its
                                own label runs).  Shapes: edt_hip_signed_supported; others: EDT_ERR_UNSUPPORTED. */
  EDT_FLAG_SMALL_WORKSPACE = 16 /* scratch = the four bit planes only (1/2 byte per voxel): passes X and Y then
                                exchange fp32 values instead of 16-bit distance indices (no 256 MiB index slab,
                                about 7 % slower at 512^3); pass it to edt_hip_workspace_bytes_flags as well */
};

/* ---- introspection -------------------------------------------------------------- */
int edt_hip_device_count(void);         /* number of visible HIP devices (0 if none)  */
/* 1 if every multiple k * wx, k <= sx + 1, is exactly representable in fp32 -- the reference's sequential fp32 sums
 * of the voxel size (src/edt.hpp:97, :113) then ARE the multiples, and pass X may hand pass Y 16-bit distance indices
 * instead of fp32 values (needs no device; exported so that tests can hold the criterion against its property). */
int edt_hip_index_form_exact(float wx, int64_t sx);
/* 1 if edt_hip_edtsq_device serves EDT_FLAG_SIGNED for this shape and these flags (needs no device) */
int edt_hip_signed_supported(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags);
const char *edt_hip_last_error(void);   /* thread-local, never NULL                   */
const char *edt_hip_version(void);

/* ---- host-buffer entry points (numpy in / numpy out) ------------------------------
 * Pointers are HOST pointers; the call stages through device memory (H2D, kernels, D2H)
 * and is synchronous.  `output` must hold one float per voxel and is fully overwritten.
 * `output` must NOT overlap `labels`: for results of 32 MiB and more, helper threads touch (write zeros into) the
 * pages of `output` while the labels are still travelling to the device, so that the copy back runs at PCIe speed.
 * For the same reason the contents of `output` are unspecified after a call that FAILED.
 * (EDT_HIP_NO_PREFAULT=1 in the environment switches the helper threads off.)
 */

/* replaces pyedt::squared_edt_1d_multi_seg<T>  (src/edt.hpp:70-119; bound at
 * src/edt.pyx:63-70).  stride must be 1 (every reference caller passes 1). */
int edt_hip_squared_edt_1d_multi_seg(const void *labels, int dtype, float *dest, int64_t n,
                                     int64_t stride, float anisotropy, int black_border);

/* replaces pyedt::_edt2dsq<T>  (src/edt.hpp:632-678, bool: :758-772; bound at
 * src/edt.pyx:72-78) */
int edt_hip_edt2dsq(const void *labels, int dtype, int64_t sx, int64_t sy, float wx, float wy,
                    int black_border, int parallel, float *output);

/* replaces pyedt::_edt3dsq<T>  (src/edt.hpp:411-484, bool: :580-587; bound at
 * src/edt.pyx:80-86) -- THE hot path. */
int edt_hip_edt3dsq(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx,
                    float wy, float wz, int black_border, int parallel, float *output);

/* replace pyedt::_edt2d<T> / _edt3d<T>  (src/edt.hpp:776-797, :591-604): the same plus a
 * correctly rounded sqrt fused into the last pass. */
int edt_hip_edt2d(const void *labels, int dtype, int64_t sx, int64_t sy, float wx, float wy,
                  int black_border, int parallel, float *output);
int edt_hip_edt3d(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx,
                  float wy, float wz, int black_border, int parallel, float *output);

/* replace pyedt::_edt2dsq_voxel_graph<T,uint8_t> / _edt3dsq_voxel_graph<T,uint8_t>
 * (src/edt_voxel_graph.hpp:54-117, :120-214; bound at src/edt.pyx:89-100).  `graph` holds
 * one byte per voxel; only bits 0x01 (+x), 0x04 (+y), 0x10 (+z) are read. */
int edt_hip_edt2dsq_voxel_graph(const void *labels, int dtype, const uint8_t *graph, int64_t sx,
                                int64_t sy, float wx, float wy, int black_border,
                                float *workspace);
int edt_hip_edt3dsq_voxel_graph(const void *labels, int dtype, const uint8_t *graph, int64_t sx,
                                int64_t sy, int64_t sz, float wx, float wy, float wz,
                                int black_border, float *workspace);

/* replaces pyedt::_binary_edt2dsq<T> / _binary_edt2d<T> / _binary_edt3dsq<T> / _binary_edt3d<T> (src/edt.hpp:681-755,
 * :487-576, :607-629 -- what edt::binary_edt / edt::binary_edtsq instantiate for ANY label type): pass X splits runs
 * at label changes like the multi-label transform, passes Y and Z do not (one envelope per column, zeros as
 * height-0 sites).  ndim in {2,3} (sz = 1 for 2-D); take_sqrt != 0: distances instead of squared distances. */
int edt_hip_binary_edtsq(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                         float wy, float wz, int black_border, int take_sqrt, float *output);

/* ---- one process, several GPUs ---------------------------------------------------------------------
 * pyedt::_edt3dsq / _edt3d on host buffers, Z-sharded over the listed devices of this process (a host thread per
 * device; X and Y passes per Z-slab in z-chunks, ONE exchange of slab records as peer-to-peer copies over xGMI --
 * the copies of a chunk run under the kernels of the next --, Z pass per Y-slab, each device copies its rows of the
 * result straight into `output`).  Same result, bit for bit, as the single-device entry points.  Device buffers and
 * streams are kept between calls (edt_hip_release_cache frees them).  The same ordinal may be listed more than once
 * (virtual devices: tests on one GPU).  Distinct ordinals must have peer access to each other: a pair without it is
 * EDT_ERR_UNSUPPORTED naming the pair (EDT_HIP_ALLOW_STAGED_PEER=1 in the environment accepts staging through host
 * memory).  A volume the slab-record form cannot cut n_devices ways (edt_hip_multi_supported == 0: sx, sy or
 * sz > 2048, fewer z-slices or 32-row words of y than devices) is EDT_ERR_UNSUPPORTED too; n_devices = 1 runs on
 * that device.
 * edt_hip_set_devices makes the ordinary host-buffer 3-D entry points (edt_hip_edt3dsq / edt_hip_edt3d, and with
 * them edt::edt<T>() and the Python / Cython front ends) take this route; every OTHER host-buffer call -- volumes that
 * cannot be cut that way (one note on stderr), 1-D and 2-D transforms, stacks of images, the binary route, the forced
 * generic kernels, sdf and the voxel-graph transforms -- runs on the FIRST listed device (the caller's current device is
 * restored afterwards); the *_device entry points are never redirected (their buffers live where the caller put them);
 * n_devices = 0 restores the current-device behaviour.  The environment variable EDT_HIP_DEVICES="0,1,2,..." presets the list. */
int edt_hip_edt3dsq_multi(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                          float wz, int black_border, int take_sqrt, float *output, const int *devices,
                          int n_devices);
int edt_hip_multi_supported(int dtype, int64_t sx, int64_t sy, int64_t sz, int n_devices);
int edt_hip_set_devices(const int *devices, int n_devices);

/* sdf / sdfsq of the reference's Python layer (src/edt.pyx:121-158, :161-202): edt(labels) - edt(labels == 0)
 * (squared != 0: edtsq(labels) - edtsq(labels == 0)) on host buffers in one round trip -- labels up once, both
 * transforms and the subtraction on the device, the difference down once.  ndim in {1,2,3}, unused extents 1. */
int edt_hip_sdf(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                float wz, int black_border, int squared, float *output);

/* The host-buffer entry points keep their device buffers (labels, output, scratch) between calls --
 * allocating gigabytes per call costs more than moving them over PCIe.  This frees them.
 * (EDT_HIP_NO_CACHE=1 in the environment disables the cache altogether.) */
int edt_hip_release_cache(void);

/* ---- device-resident entry points --------------------------------------------------
 * All pointers are DEVICE pointers on the current HIP device; `stream` is a hipStream_t
 * (NULL = the null stream).  Calls only enqueue work (no host synchronisation, no
 * allocation), so they can be timed with events and captured into a hipGraph.
 *
 * Alignment.  Label, field and output pointers (d_labels, d_output, d_dt, d_features, d_out, d_partial, d_graph, masks ...)
 * need the alignment of their element type and nothing more: a view at any element offset into a larger buffer is served,
 * with the same results bit for bit (the kernels choose their vector forms by the address and fall back element by
 * element).  Count and table outputs (d_n, d_counts, d_keys ...) likewise need their element's alignment.  The slab-record
 * forms state their own 8- and 16-byte requirements below.
 * d_workspace is the one exception: every *_device entry point that takes one requires it 256-BYTE ALIGNED and refuses
 * any other pointer with EDT_ERR_BAD_ARG before any device work.  256 bytes is the granule the scratch is carved at -- the
 * bit planes, parent words and tables carved from it are targets of 32- and 64-bit atomics and of 16-byte loads, all relative
 * to the base -- and it is what hipMalloc (and torch's allocator) deliver; every caller in this tree passes such a base.
 *
 * Workspace.  The workspace of every *_device entry point is initialised by the call itself; a reused one needs no memset.
 * A call reads nothing of its scratch that it has not written on `stream` before: what an earlier call -- of another shape,
 * of other flags, another entry point's -- or the caller left there never shows in a result.  Nothing is kept in a workspace
 * between calls either.  Every word a call sets it sets with kernels on `stream`, so a captured call replays like the call
 * itself, on whatever the workspace holds by then.  (tests/test_gpu_workspace_contract.py; DESIGN.md 13 lists the regions.)
 */

/* bytes of scratch edt_hip_edtsq_device needs for a volume of this shape: the four bit planes of the column
 * passes (1/8 of a byte per voxel each: 0.5 GiB for 1024^3) plus one slab of 16-bit distance indices between
 * passes X and Y (2 bytes per voxel, never more than 256 MiB: larger volumes run those passes slab by slab).
 * Only a call that has to use the size-agnostic column kernels (an axis longer than 32735 voxels, or
 * EDT_FLAG_FORCE_GENERIC) needs a second fp32 volume and the hull stacks as well (+ 8 bytes per voxel): ask
 * with the flags of the call.  A call carves its regions from the base of whatever it is given, by its own flags: one buffer
 * of the largest size -- the maximum of edt_hip_workspace_bytes_flags over the flag sets in use -- serves calls of every
 * flag set, in any order, without being cleared in between. */
size_t edt_hip_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
size_t edt_hip_workspace_bytes_flags(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags);

/* A stack of `count` independent 2-D images, images[k][y][x] (pyedt::_edt2dsq per image, src/edt.hpp:632-678):
 * one launch per pass for the whole stack, so that small images fill the chip (a single 512 x 512 image is 16
 * workgroups on 256 compute units).  Host buffers; take_sqrt != 0 gives edt instead of edtsq.  The device-resident
 * form is edt_hip_edtsq_device(ndim = 3, sz = count, flags | EDT_FLAG_BATCH_2D). */
int edt_hip_edt2dsq_batch(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t count, float wx, float wy,
                          int black_border, int take_sqrt, float *output);

/* ndim in {1,2,3}; unused extents must be 1.  flags: EDT_FLAG_*.  d_output may not alias
 * d_labels.  Implements _edt3dsq / _edt2dsq / squared_edt_1d_multi_seg (+ optional sqrt).
 * ndim = 1: with edt_hip_workspace_bytes() of scratch the line runs through the parallel pipeline (a thread per
 * voxel); with d_workspace = NULL (or too small) it is served by one thread walking the line -- correct, and slow
 * for long lines.
 * Enqueue-only on `stream`; the workspace is initialised by the call itself; a reused one needs no memset. */
int edt_hip_edtsq_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy,
                         int64_t sz, float wx, float wy, float wz, int flags, float *d_output,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/* Per-pass timing hook for bench.py: when enabled, edt_hip_edtsq_device brackets every
 * kernel it launches with hipEvents on `stream`.  After synchronising the stream,
 * edt_hip_get_pass_times copies the durations (ms) of the last call, in launch order,
 * into `ms` and returns how many there were (names via edt_hip_get_pass_name). */
int edt_hip_set_profiling(int enabled);
/* Diagnostics / test hook.  The mode belongs to the CALLING THREAD (EDT_HIP_DEBUG_MODE in the environment presets
 * every thread's).  The shipped library honours only bits that choose between result-preserving forms of the same
 * computation -- e.g. 0x2000: no tile of the column pass takes the windowed path, 0x4000: every tile does, 0x8000:
 * fp64 candidates there (0x2000000: only where fp32 fma candidates would serve), 0x100000: fp32 instead of 16-bit indices between passes X and Y, 0x20000: up-sampled
 * voxel-graph formulation, 32 / 64: workgroup-phased row / column kernels (csrc/edt_common.h lists them); results
 * are bit-identical under every one of them, which is what the GPU test tier uses them for.  Bits that switch
 * phases off (wrong results, for cost measurements) exist only in a build with -DEDT_DIAG and are ignored here.
 * edt_hip_get_debug_mode returns the effective (masked) mode of the calling thread. */
int edt_hip_set_debug_mode(int mode);
int edt_hip_get_debug_mode(void);
/* Diagnostics (pure host arithmetic, no device needed): the library's own proof that the 16-bit integer column kernel
 * (csrc/edt_colq16.hip) can refuse no tile of pass Y / pass Z of a call of these extents and voxel sizes whose pass X hands
 * over 16-bit distance indices -- where it holds, the fp32 launch over the hand-over list is not made.  Returns 0 if the
 * voxel sizes share no quantum (the integer kernel does not apply), 1 otherwise with *pass_y / *pass_z set to 0 / 1 (pass_z:
 * behind a pass Y that holds; always 0 for ndim == 2).  The CPU test tier plays both passes through the kernel's lane logic
 * and holds this answer against what the tiles do (tests/test_q16_logic.py).  No counterpart in the reference. */
int edt_hip_q16_no_refusals(int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, int ndim, int black_border,
                            int *pass_y, int *pass_z);
/* Diagnostics (pure host arithmetic, no device needed): the ROUTE of an edt_hip_edtsq_device call -- everything the library
 * decides before its first launch: which kernels run, in which order, and what lives in which part of the workspace.  The
 * call itself asks the same function and then only executes the answer (csrc/edt_api.hip: route_of, run_device; DESIGN.md,
 * "The route of a call").  Inputs besides the call's own: the calling thread's debug mode, EDT_HIP_FORCE_GENERIC,
 * EDT_HIP_WHOLE_INDEX_BYTES and EDT_HIP_PLANE_PAD_BYTES in the environment, the bytes of the workspace the caller brings
 * (SIZE_MAX: whatever the route asks for; 0: none) and d_output's address modulo 16 (out_misalignment: the integer column
 * kernel loads 16-byte granules of the field).  Returns EDT_OK and the route, or what the call would refuse with before it
 * launches anything -- same code, same edt_hip_last_error() -- and a route of zeros; an empty volume is EDT_OK and zeros. */
enum {
  EDT_ROUTE_X_REGISTER = 0, /* rows in registers, one to four waves per row (csrc/edt_rowwave.hip)            */
  EDT_ROUTE_X_PHASED = 1,   /* the workgroup-phased row kernel (csrc/edt_rows.hip)                            */
  EDT_ROUTE_X_LINE = 2,     /* the line pipeline, a thread per voxel: rows no row kernel takes, 1-D lines     */
  EDT_ROUTE_X_SERIAL = 3    /* a thread per row: forced generic, and a 1-D line without a workspace           */
};
enum {
  EDT_ROUTE_COL_NONE = 0,         /* the call has no such pass                                                  */
  EDT_ROUTE_COL_SERIAL = 1,       /* the size-agnostic kernel, from one volume into the other (ping-pong)       */
  EDT_ROUTE_COL_FP32 = 2,         /* in place, an fp32 kernel over every tile                                   */
  EDT_ROUTE_COL_INTEGER_LIST = 3, /* in place, the 16-bit integer kernel, then an fp32 kernel over its list     */
  EDT_ROUTE_COL_INTEGER_ALONE = 4 /* the integer kernel alone: the host has proven that it refuses no tile      */
};
typedef struct edt_hip_route {
  int32_t x_kernel;           /* EDT_ROUTE_X_*: the kernel of pass X                                                          */
  int32_t planes_from_labels; /* 1: the run bit planes of y and z are built from the labels by passes of their own (y_bits,
                                 z_bits); 0: the row kernel emits them and z_bits is their transposition (1-D: no planes)     */
  int32_t index_form;         /* 1: pass X hands pass Y 16-bit distance indices, slab by slab, instead of fp32 values         */
  int32_t codes_whole;        /* 1: the index buffer holds every slice of the volume, 0: one slab (or does not exist)         */
  int32_t y_pass, z_pass;     /* EDT_ROUTE_COL_*                                                                              */
  int32_t plane16;            /* 1: pass Y leaves its results in the index buffer as 16-bit values, pass Z reads them there   */
  int32_t plane_inf_ok;       /* 1: ... and a tile of nothing but +inf may stay in that plane (pass Z carries +inf)           */
  int32_t skip_nz;            /* 1: nobody reads a foreground plane; pass X writes none, z_bits moves the run starts only     */
  int32_t row_flags;          /* 1: ... and its storage holds the row flags: pass X stores no indices of rows without a run start */
  int32_t zero_label;         /* what label 0 is to pass X: 0 background; 1 a label like any other, all-ones foreground
                                 planes; 2 a label like any other, true foreground planes (for the sign epilogue)            */
  int32_t sign;               /* EDT_FLAG_SIGNED: 0 not asked for, 1 the epilogue of pass Z, 2 a pass of its own ("sign")     */
  int32_t binary_yz;          /* 1: one run per column in y and z (EDT_FLAG_BINARY_YZ on a label type that is not bool)       */
  int32_t first_buffer;       /* where pass X writes: 0 d_output, 1 the second volume (an odd number of ping-pong passes)     */
  int32_t second_volume;      /* 1: the workspace holds a second fp32 volume and the hull stacks of the serial column kernel  */
  int32_t index_fallback;     /* 1: the workspace brought is too small for the index buffer and large enough without it: the
                                 route is the one of EDT_FLAG_SMALL_WORKSPACE (slab = 0)                                      */
  int64_t slab;               /* slices per slab of the index buffer (0: there is none)                                       */
  int64_t slabs;              /* launches of pass X and of pass Y each: slabs of the index form, else 1                       */
  int64_t code_pitch;         /* elements between the slices of the index buffer and of the 16-bit plane (0: 1-D)            */
  uint64_t workspace_bytes;   /* what this route needs = edt_hip_workspace_bytes_flags, or less under index_fallback          */
} edt_hip_route;
int edt_hip_transform_route(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, int flags,
                            size_t workspace_bytes, uint32_t out_misalignment, edt_hip_route *route);
int edt_hip_get_pass_times(float *ms, int capacity);
const char *edt_hip_get_pass_name(int index);

/* ---- Z-sharded (multi-GPU) building blocks ------------------------------------------
 * One process per GPU holds a contiguous Z-slab.  Phase 1 runs the X and Y passes on the
 * slab (no data dependence across z) and emits, per voxel, the fp32 partial result plus
 * one flag byte (bit0 = foreground, bit1 = label differs from the voxel below in z).
 * The host layer then re-partitions both arrays from Z-slabs to Y-slabs with ONE
 * all-to-all (RCCL over xGMI) and phase 2 runs the Z pass on whole z-columns.
 *   d_halo: the last xy-slice of the previous rank's labels (NULL on the first rank) --
 *           the one-slab halo that decides run continuity across the cut.
 * Both phases, in every form below: enqueue-only on `stream`; the workspace is initialised by the call itself; a reused one
 * needs no memset (one buffer may serve the XY phase and the Z phase in turn).
 */
size_t edt_hip_shard_workspace_bytes(int dtype, int64_t sx, int64_t sy, int64_t sz);
int edt_hip_shard_xy_device(const void *d_labels, const void *d_halo, int dtype, int64_t sx,
                            int64_t sy, int64_t sz_local, float wx, float wy, int flags,
                            float *d_partial, uint8_t *d_zflags, void *d_workspace,
                            size_t workspace_bytes, void *stream);
int edt_hip_shard_z_device(float *d_partial, const uint8_t *d_zflags, int64_t sx,
                           int64_t sy_local, int64_t sz, float wz, int flags,
                           void *d_workspace, size_t workspace_bytes, void *stream);
/* The same with `field_floor`: a lower bound of the NON-ZERO values of the partial field, which the caller of both
 * phases knows -- after edt_hip_shard_xy_* every non-zero value is at least min(fl32(wx*wx), fl32(wy*wy))
 * (edt_hip_field_floor).  It lets the Z pass form its candidates in fp32 for voxel sizes whose multiples are not exact
 * in fp32; results are the same bits either way.  0 (or anything not positive) = unknown, which is
 * what the entry points without the argument pass.  A floor ABOVE a non-zero value of the field is a contract
 * violation (results may differ from the reference's in the last bit). */
float edt_hip_field_floor(float wx, float wy);
int edt_hip_shard_z_device_ex(float *d_partial, const uint8_t *d_zflags, int64_t sx,
                              int64_t sy_local, int64_t sz, float wz, float field_floor, int flags,
                              void *d_workspace, size_t workspace_bytes, void *stream);

/* Slab records: the fast form of the same two phases (sx, sy and sz <= 2048; query with
 * edt_hip_shard_records_supported, otherwise use the pair above).  The y axis is cut into `nparts`
 * destination ranges at multiples of 32 rows (y_splits[0] = 0 ... y_splits[nparts] = sy, HOST array).
 * For destination h and every xy-slice of the slab the XY phase writes ONE contiguous record of
 * edt_hip_shard_record_floats(sx, ylen_h) 4-byte elements straight into d_blocks[h] (device pointer
 * to sz_local consecutive records; HOST array of nparts pointers):
 *     ylen_h * sx floats   the slice after the X and Y passes, rows of that destination only
 *     words_h * sx uint32  foreground bits, 32 rows of y per word      (words_h = ceil(ylen_h / 32))
 *     words_h * sx uint32  "label differs from the voxel below in z" bits, same packing
 * i.e. 4.25 bytes per voxel travel instead of the labels, each peer's message is contiguous on
 * both sides (no pack / unpack copies), and a rank may hand in its OWN part of the receive buffer
 * as d_blocks[rank].  A slab can be processed in z-chunks (d_halo of a later chunk = the last
 * slice of the previous one) so that the exchange of one chunk overlaps the kernels of the next.
 * The Z phase takes the gathered buffer of sz records (all z, this rank's rows) and leaves the result
 * in the float part of every record: row (z, y) starts at d_records + z * record_floats + y * sx. */
int edt_hip_shard_records_supported(int dtype, int64_t sx, int64_t sy, int64_t sz);
size_t edt_hip_shard_record_floats(int64_t sx, int64_t y_rows);
size_t edt_hip_shard_records_workspace_bytes(int dtype, int64_t sx, int64_t sy, int64_t sz);
int edt_hip_shard_xy_records_device(const void *d_labels, const void *d_halo, int dtype, int64_t sx,
                                    int64_t sy, int64_t sz_local, float wx, float wy, int flags,
                                    int nparts, const int64_t *y_splits, void *const *d_blocks,
                                    void *d_workspace, size_t workspace_bytes, void *stream);
int edt_hip_shard_z_records_device(float *d_records, int64_t sx, int64_t sy_local, int64_t sz,
                                   float wz, int flags, void *d_workspace, size_t workspace_bytes,
                                   void *stream);
int edt_hip_shard_z_records_device_ex(float *d_records, int64_t sx, int64_t sy_local, int64_t sz,
                                      float wz, float field_floor, int flags, void *d_workspace,
                                      size_t workspace_bytes, void *stream);
/* The same for a caller that names all three voxel sizes (the ones of the XY phase that produced the records and this
 * phase's): field_floor = edt_hip_field_floor(wx, wy), and where the three sizes share a quantum ((1,1,1), (6,6,30) ...)
 * the pass runs on the 16-bit integer column kernel (csrc/edt_colq16.hip); the same bits either way. */
int edt_hip_shard_z_records_device_w(float *d_records, int64_t sx, int64_t sy_local, int64_t sz, float wx, float wy,
                                     float wz, int flags, void *d_workspace, size_t workspace_bytes, void *stream);

/* Slab records of 16-BIT values (2.25 bytes per voxel over the links instead of 4.25).  Where the three voxel sizes share a
 * quantum (csrc/edt_colq16.hip: w_i^2 = a_i q) and both column axes fit the integer kernel (97..1024 rows), the Y pass's
 * results are integers N < 2^16 in quanta: the record of destination h and slice z is then
 *     ylen_h * sx 16-bit values (row-major, as packed pairs)  |  the two bit planes as above
 * = edt_hip_shard_record16_words(sx, ylen_h) 4-byte words (an even number: blocks are 8-byte aligned, the gathered buffer and
 * d_out 16-byte).  edt_hip_shard_records16_supported: the extents of the WHOLE volume
 * and its voxel sizes allow it.  A tile the integer kernel cannot take (values beyond 16 bits, rows without any boundary)
 * has no 16-bit form: the XY phase adds the number of such tiles to *d_refused -- a device counter the caller zeroes and
 * reads -- and leaves their rows unspecified; a caller that finds it non-zero repeats the step with the fp32 records
 * (edt/distributed.py: the ranks agree on it with one all-reduce of the counter, off the critical path).  The Z phase reads
 * the gathered records (sz x record16 words) and writes the dense (sz, sy_local, sx) fp32 result to d_out; the same bits as
 * every other route.  No counterpart in the reference (src/edt.hpp:448-475 is what both phases replace).
 * (*d_refused is the caller's word, not scratch: the XY phase only adds to it.) */
int edt_hip_shard_records16_supported(int dtype, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz);
size_t edt_hip_shard_record16_words(int64_t sx, int64_t y_rows);
int edt_hip_shard_xy_records16_device(const void *d_labels, const void *d_halo, int dtype, int64_t sx, int64_t sy,
                                      int64_t sz_local, float wx, float wy, float wz, int flags, int nparts,
                                      const int64_t *y_splits, void *const *d_blocks, uint32_t *d_refused, void *d_workspace,
                                      size_t workspace_bytes, void *stream);
int edt_hip_shard_z_records16_device(const void *d_records, float *d_out, int64_t sx, int64_t sy_local, int64_t sz, float wx,
                                     float wy, float wz, int flags, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- fused helpers on device-resident data ------------------------------------------ */
/* out[i] = a[i] - b[i]  (src/edt.pyx:156-158, sdf = edt(x) - edt(x == 0)) */
int edt_hip_subtract_device(const float *d_a, const float *d_b, float *d_out, int64_t count,
                            void *stream);
/* pyedt::extract_runs (src/edt_voxel_graph.hpp:238-268) on device-resident labels: the START offsets of the
 * maximal constant runs of the flattened array, ascending (run k = [starts[k], starts[k+1]) resp. up to count for
 * the last one; its label is labels[starts[k]]).  *d_count receives the number of runs; at most `capacity` starts are
 * written (capacity = 0, d_starts = NULL: count only).  Enqueue-only; scratch: edt_hip_runs_workspace_bytes -- initialised
 * by the call itself; a reused one needs no memset. */
size_t edt_hip_runs_workspace_bytes(int64_t count);
int edt_hip_extract_runs_device(const void *d_labels, int dtype, int64_t count, int64_t *d_starts, int64_t capacity,
                                int64_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream);

/* mask[i] = (labels[i] == 0) as one byte per voxel (the `data == 0` of src/edt.pyx:157) */
int edt_hip_is_background_device(const void *d_labels, int dtype, uint8_t *d_mask, int64_t count,
                                 void *stream);

/* pyedt::_edt2dsq_voxel_graph / _edt3dsq_voxel_graph (src/edt_voxel_graph.hpp:54-117, :120-214) on
 * device-resident data: labels, graph (one byte per voxel, bits as in the host entry points above) and
 * output live in HBM; enqueue-only on `stream`.  Scratch: edt_hip_voxel_graph_workspace_bytes (native form: the
 * even-x cells of the doubled grid as fp32, 4 x voxels floats, and the bit planes of its two column passes; the
 * up-sampled fallback for doubled axes beyond 2048 rows: the 2x uint8 volume, its fp32 transform and the
 * ordinary workspace of that volume).  The workspace is initialised by the call itself; a reused one needs no memset. */
size_t edt_hip_voxel_graph_workspace_bytes(int ndim, int64_t sx, int64_t sy, int64_t sz);
int edt_hip_edtsq_voxel_graph_device(const void *d_labels, int dtype, const uint8_t *d_graph, int ndim,
                                     int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                                     int flags, float *d_output, void *d_workspace, size_t workspace_bytes,
                                     void *stream);

/* out[i] = (labels[i] == *key) ? dt[i] : 0 -- the image edt.each() yields for one label
 * (src/edt.pyx:950-994: zeros + transfer of the label's runs, src/edt_voxel_graph.hpp:290-310), as one
 * streaming kernel on device-resident data.  `key` is a HOST pointer to one value of the label dtype. */
int edt_hip_select_label_device(const void *d_labels, int dtype, const float *d_dt, const void *key,
                                float *d_out, int64_t count, void *stream);

/* ---- feature transform (nearest-boundary indices) and expand_labels ------------------------------------------------
 * Conventions as above: x fastest, idx = x + sx * (y + sy * z), label 0 is background, labels compared at full width with
 * their type's == (so -0.0 is background and a NaN voxel differs from every voxel).  With the squared voxel sizes
 * D(p,q) = wx^2 (px-qx)^2 + wy^2 (py-qy)^2 + wz^2 (pz-qz)^2:
 *   - foreground voxel p of label L != 0: its FEATURE is a voxel q with label(q) != L that minimises D(p,q); edtsq(p) is
 *     that minimum.  With black_border the one-voxel shell around the volume counts as label 0, so one component (at most)
 *     may be -1 or s_axis;
 *   - background voxel: its feature is itself;
 *   - no feature (black_border off and the whole volume one label): every component is -1.
 * Tie rule, separable, pass by pass in the order X, Y, Z: among the candidates of minimal pass value, the one with the
 * smallest coordinate along that pass's axis.
 *   pass X: for p in the x-run [a,b], the candidates are a-1 (if a > 0 or black border) and b+1 (likewise); a tie takes a-1;
 *   pass Y: the rows j of p's y-run with a finite pass-X value, with feature (fx(j), j), and the border sites a-1 and b+1,
 *           which are their own feature (x, j);
 *   pass Z: the same, carrying (fx, fy).
 * Where the voxel sizes share a quantum (w_i^2 = a_i q, small integers a_i: (1,1,1), (6,6,30), (4,4,40), (0.5,0.5,1) ...)
 * the pass values are exact integers (64-bit), so the features are fully determined by the rule.  Otherwise the passes
 * run in fp64 and the feature satisfies D(p, f(p)) <= (1 + 2^-20) min_q D(p,q).  The same call gives the same output
 * (no atomics decide a winner).  Limits: extents up to 2^31 - 1 per axis (features are int32), volumes past 2^31 voxels. */

/* Scratch of edt_hip_feature_transform_device: 4 bytes per voxel for ndim = 1, 24 for ndim = 2, 40 for ndim = 3 (pass
 * values, carried coordinates, hull stacks).  0 for a bad shape or flags. */
size_t edt_hip_feature_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags);
/* d_features: ndim planes of sx*sy*sz int32 each -- plane 0 the x coordinate of the feature, plane 1 y, plane 2 z.
 * flags: EDT_FLAG_BLACK_BORDER, EDT_FLAG_FORCE_GENERIC (accepted; every axis length runs on the size-agnostic column
 * kernel, so the features are the same); any other flag is EDT_ERR_UNSUPPORTED.  ndim 1..3, unused extents 1, voxel
 * sizes as for edt_hip_edtsq_device (EDT_ERR_BAD_ARG before any device work).  NULL pointers and a missing or too small
 * workspace are EDT_ERR_BAD_ARG.  Enqueue-only on `stream`: no allocation, no synchronisation; the workspace is initialised
 * by the call itself (a reused one needs no memset). */
int edt_hip_feature_transform_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                                     float wy, float wz, int flags, int32_t *d_features, void *d_workspace,
                                     size_t workspace_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device).  `features` holds ndim * sx*sy*sz int32. */
int edt_hip_feature_transform(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                              float wy, float wz, int black_border, int32_t *features);

/* expand_labels: out = labels; for each background voxel p, with f the feature of p in the feature transform of the mask
 * labels == 0 (black border off): out[p] = labels[f] if f exists and D(p,f) <= distance^2, where
 *   D = (fl64(wx^2 dx^2) + fl64(wy^2 dy^2)) + fl64(wz^2 dz^2)
 * in fp64 from the integer offsets and the fp32 voxel sizes widened to fp64 (no fma); otherwise out[p] keeps its own
 * (background) value.  No foreground at all: out is a copy of labels.  distance >= 0, +inf allowed; NaN or negative is
 * EDT_ERR_BAD_ARG.  The output has the labels' dtype and may not alias them.  Scratch: one byte per voxel for the mask
 * plus the feature transform's workspace of the mask -- initialised by the call itself; a reused one needs no memset.
 * Enqueue-only on `stream`. */
size_t edt_hip_expand_labels_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
int edt_hip_expand_labels_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                                 float wy, float wz, double distance, void *d_out, void *d_workspace, size_t workspace_bytes,
                                 void *stream);
int edt_hip_expand_labels(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                          float wz, double distance, void *output);

/* ---- label_stats: per-label count, maximum of a field, its argmax and the bounding box ------------------------------
 * Conventions as above: x fastest, idx = x + sx * (y + sy * z), label 0 is background, labels compared at full width with
 * their type's ==.  `dt` is any NaN-free fp32 field of the labels' shape (+inf and negative values included: edt without a
 * black border, sdf).  The table has one entry for each distinct non-zero label L:
 *   key     L, in the labels' dtype (signed integers as their unsigned bit patterns, as everywhere at this ABI);
 *   count   the number of voxels with label L (int64);
 *   max     the largest dt over those voxels (fp32);
 *   argmax  the smallest idx among the label's voxels whose dt equals max (int64);
 *   bbox    inclusive min and max of x, y and z over the label's voxels: int32 x 6 in the order x0,x1,y0,y1,z0,z1
 *           (unused axes 0,0).
 * Floating-point labels: -0.0 is background; a NaN voxel equals nothing, so it belongs to no label, has no entry and is in
 * no count.  Bool: one label, any non-zero byte is key 1.  If dt holds NaN, the max and argmax of the labels it touches are
 * unspecified (nothing faults).
 * Order: ascending key -- unsigned order for integers, numeric order for floats.
 * Determinism: the same call gives the same table, bit for bit (integer min / max / add atomics over an order-preserving
 * map of dt; nothing depends on which thread won a hash slot).
 * Capacity: the output arrays hold max_labels entries (bbox: 6 * max_labels).  With at most max_labels distinct non-zero
 * labels *n_labels is their number and the table is complete.  Otherwise *n_labels is SOME value greater than max_labels,
 * the arrays' contents are unspecified and the call still returns EDT_OK: the caller retries with more room.
 * Sizes: offsets are 64-bit throughout (volumes past 2^32 voxels). */

/* Scratch of edt_hip_label_stats_device: nothing per voxel; the label table -- 256 / 65536 direct-indexed slots for 8- /
 * 16-bit labels, else an open-addressing hash table of the power of two >= max(1024, 2 * max_labels) slots, 52 bytes per
 * slot, plus 8 bytes per label (a max_labels above `voxels` counts as `voxels`).  0 for a bad dtype or max_labels < 1. */
size_t edt_hip_label_stats_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels);
/* ndim 1..3, unused extents 1, max_labels >= 1; NULL pointers and a missing or too small workspace are EDT_ERR_BAD_ARG
 * before any device work.  Enqueue-only on `stream`: no allocation, no synchronisation; the workspace is cleared by the call
 * itself (a reused one needs no memset).  d_n_labels: one int64 on the device. */
int edt_hip_label_stats_device(const void *d_labels, int dtype, const float *d_dt, int ndim, int64_t sx, int64_t sy,
                               int64_t sz, int64_t max_labels, void *d_keys, int64_t *d_counts, float *d_max,
                               int64_t *d_argmax, int32_t *d_bbox, int64_t *d_n_labels, void *d_workspace,
                               size_t workspace_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device).  dt: a HOST field, or NULL: the ordinary transform of the labels with
 * these voxel sizes and this border rule runs on the device first (distances, i.e. with sqrt: edt_hip_edt3d's field; the
 * voxel-size rules above apply) and never leaves it.  Only the table is copied back. */
int edt_hip_label_stats(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                        float wz, int black_border, const float *dt, int64_t max_labels, void *keys, int64_t *counts,
                        float *max, int64_t *argmax, int32_t *bbox, int64_t *n_labels);

/* ---- label_moments: exact raw moments, centroid and covariance of every label ----------------------------------------
 * Conventions, keys, order, capacity, *n_labels and overflow behaviour are label_stats': x fastest, idx = x + sx * (y + sy * z),
 * label 0 is background, integers at full width, bool: any non-zero byte is key 1, -0.0 is background, a NaN voxel belongs to
 * no label; ascending key; the arrays hold max_labels entries (sums 9 *, centroid 3 *, central 6 * max_labels), and with
 * more distinct labels *n_labels is SOME value greater than max_labels, the contents are unspecified and the call returns
 * EDT_OK.  The table has one entry for each distinct non-zero label L, over the voxels p = (x, y, z) with label L:
 *   key       L, in the labels' dtype;
 *   count     n, the number of those voxels (int64);
 *   sums      nine int64 in the order Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz: the raw moments about the volume's origin in
 *             voxel index units (Sxy = sum of x * y ...), exact;
 *   centroid  three fp64: fl(fl(S_a) / fl(n)) -- fl of a 64-bit integer is its one round-to-nearest-even conversion, the
 *             division is IEEE binary64; unused axes give 0.0;
 *   central   six fp64 in the order xx, yy, zz, xy, xz, yz: the population covariance in voxel units,
 *             fl(fl(fl(M_ab) / fl(n)) / fl(n)) with M_ab = n * S_ab - S_a * S_b taken EXACTLY as a signed 128-bit integer and
 *             converted once, round to nearest even, its sign apart.  Nothing subtracts two rounded numbers: an elongated
 *             object far from the origin gets the relative accuracy of one at the origin.
 * Determinism: the same call gives the same table, bit for bit (64-bit integer adds and a compare-and-swap on the key).
 * Range: a volume with voxels * (E - 1)^2 >= 2^63, E the largest extent, is refused with EDT_ERR_UNSUPPORTED before any
 * device work (outputs and scratch untouched; the test is made in 128-bit arithmetic).  Below the bound every sum fits int64
 * and every M_ab 128 bits.  Every 3-D shape the tiled kernels accept is far inside; only lines of millions of voxels are not. */

/* Scratch of edt_hip_label_moments_device: nothing per voxel; label_stats' tables with wider slots -- 256 / 65536
 * direct-indexed slots for 8- / 16-bit labels, else an open-addressing hash table of the power of two >= max(1024,
 * 2 * max_labels) slots; 88 bytes per slot (the key and ten 64-bit sums), plus 8 bytes per label (a max_labels above
 * `voxels` counts as `voxels`).  0 for a bad dtype or max_labels < 1. */
size_t edt_hip_label_moments_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels);
/* ndim 1..3, unused extents 1, max_labels >= 1; NULL pointers and a missing, too small or misaligned scratch (d_scratch is
 * the call's workspace: 256-byte aligned, at least the query's bytes) are EDT_ERR_BAD_ARG before any device work.
 * Enqueue-only on `stream`: no allocation, no synchronisation; the scratch is cleared by the call itself (a reused one needs
 * no memset), so the call can be captured.  d_n_labels: one int64 on the device. */
int edt_hip_label_moments_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                 int64_t max_labels, void *d_keys, int64_t *d_counts, int64_t *d_sums /* 9*max_labels */,
                                 double *d_centroid /* 3*max_labels */, double *d_central /* 6*max_labels */,
                                 int64_t *d_n_labels, void *d_scratch, size_t scratch_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device).  The labels cross once; only the table is copied back. */
int edt_hip_label_moments(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels,
                          void *keys, int64_t *counts, int64_t *sums, double *centroid, double *central, int64_t *n_labels);

/* ---- label_topology: exact Euler numbers and surface of every label --------------------------------------------------
 * Conventions, keys, order, capacity, *n_labels and overflow behaviour are label_moments': x fastest, idx = x + sx * (y + sy * z),
 * label 0 is background, integers at full width, bool: any non-zero byte is key 1, -0.0 is background, a NaN voxel belongs to
 * no label; ascending key; the arrays hold max_labels entries (closed and interior 8 * max_labels each), and with more
 * distinct labels *n_labels is SOME value greater than max_labels, the contents are unspecified and the call returns EDT_OK.
 * Cells: a CELL of a voxel p is given by c in {-1, 0, +1}^3 -- the voxel's 8 vertices, 12 edges, 6 faces and the cube itself.
 *   Its TYPE is the set of axes with c_a = 0, the axes it extends along: a 3-bit index, bit 0 = x, bit 1 = y, bit 2 = z.  Its
 *   INCIDENT voxels are p + e with e_a in {0, c_a}.  Positions outside the volume hold no label: there is no border option,
 *   the volume's edge ends an object, and the object's boundary cells there count.
 * The table has one entry for each distinct non-zero label L:
 *   key       L, in the labels' dtype;
 *   closed    eight int64, closed[S] = the number of distinct cells of type S with AT LEAST ONE incident voxel of label L: the
 *             closed cubical complex of L (26-adjacency in 3-D, 8-adjacency in 2-D);
 *   interior  eight int64, interior[S] = the number of cells of type S whose incident voxels ALL carry L: the open set
 *             (6- and 4-adjacency).  interior[7] = closed[7] = the voxel count.
 * Always the 3-D slab: unused extents are 1.  For a missing axis a, the count of type S of the lower-dimensional image is the
 *   slab's count of type S with bit a set: closed cells transverse to an axis of extent 1 come in two identical copies, interior
 *   cells transverse to it are 0.  The Euler number of the slab equals that of the image.
 * Derived, with |S| the cell's dimension and nd = 3 for the slab:
 *   euler, full adjacency   sum over S of (-1)^|S| * closed[S]            (components - tunnels + cavities)
 *   euler, face adjacency   sum over S of (-1)^(nd - |S|) * interior[S]
 *   intrinsic volumes for voxel sizes w:  V_j = sum over S of (-1)^(|S| - j) * closed[S] * e_j(w_a : a in S), e_j the elementary
 *     symmetric polynomial: V_nd the volume, 2 * V_(nd-1) the area of the exposed voxel faces (the perimeter in 2-D), V_1 the
 *     mean-breadth functional, V_0 the Euler number.  The face area does not converge to a smooth surface's area (about 1.5
 *     times larger for a ball); it is exact and additive.
 * Counting: a voxel owns a cell for L when it is the first incident voxel with label L in memory order, so every cell is
 *   counted once; the counts do not depend on that order.  The largest count is 8 * voxels.
 * Determinism: the same call gives the same table, bit for bit (integer adds and a compare-and-swap on the key). */

/* Scratch of edt_hip_label_topology_device: nothing per voxel; label_moments' tables with wider slots -- 256 / 65536
 * direct-indexed slots for 8- / 16-bit labels, else an open-addressing hash table of the power of two >= max(1024,
 * 2 * max_labels) slots; 136 bytes per slot (the key and sixteen 64-bit counts), plus 8 bytes per label (a max_labels above
 * `voxels` counts as `voxels`).  0 for a bad dtype or max_labels < 1. */
size_t edt_hip_label_topology_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels);
/* ndim 1..3, unused extents 1, max_labels >= 1; NULL pointers and a missing, too small or misaligned scratch (d_scratch is
 * the call's workspace: 256-byte aligned, at least the query's bytes) are EDT_ERR_BAD_ARG before any device work, in this
 * order: dtype, ndim, unused extents, max_labels, d_n_labels, the other pointers, the scratch.  Enqueue-only on `stream`: no
 * allocation, no synchronisation; the scratch is cleared by the call itself (a reused one needs no memset), so the call can
 * be captured.  d_n_labels: one int64 on the device. */
int edt_hip_label_topology_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                  int64_t max_labels, void *d_keys, int64_t *d_closed /* 8*max_labels */,
                                  int64_t *d_interior /* 8*max_labels */, int64_t *d_n_labels, void *d_scratch,
                                  size_t scratch_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device).  The labels cross once; only the table is copied back. */
int edt_hip_label_topology(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels,
                           void *keys, int64_t *closed, int64_t *interior, int64_t *n_labels);

/* ---- connected components: multi-label component labelling on the device ---------------------------------------------
 * Conventions as above: x fastest, idx = x + sx * (y + sy * z), label 0 is background.
 * Adjacency: connectivity = c, 1 <= c <= ndim.  Two voxels are neighbours if their coordinates differ by at most 1 along
 *   every axis, and along at most c axes: 1-D 2 neighbours; 2-D 4 (c = 1) or 8 (c = 2); 3-D 6, 18 or 26.
 * Connection: neighbours p, q are connected iff label(p) == label(q) and label(p) != 0 -- compared at full width with the
 *   type's ==, as everywhere.  Floats: -0.0 is background; a NaN voxel is foreground and equals nothing, so it is a
 *   component of its own.  EDT_BOOL: any non-zero byte is the one foreground label (bytes 1 and 2 join).  binary != 0:
 *   every non-zero voxel is one class, for every dtype (scipy.ndimage.label of data != 0; NaN is non-zero).
 * Output: one uint32 per voxel -- 0 where the label is background, otherwise the component's number in 1..N.  Components
 *   are numbered in ascending order of the smallest idx among their voxels (raster order of first encounter along the
 *   memory order).  *n receives N as int64.
 * Determinism: the same call gives the same output, bit for bit.  Which thread wins an atomic may decide the shape of the
 *   intermediate union-find forest, never the result: the root of a component is its smallest idx, and that is unique.
 * Limits: sx * sy * sz <= 2^31 - 1 (parents and numbers are 32-bit; a root carries its number with the top bit set until
 *   the last sweep strips it).  For a larger volume the workspace query returns 0 and the entry points return
 *   EDT_ERR_UNSUPPORTED; the check is made in 64-bit arithmetic before any device work.  Byte offsets are 64-bit. */

/* Scratch of edt_hip_connected_components_device: the output array itself serves as the parent array of the union-find,
 * so nothing per voxel -- one uint32 for every 2048 voxels (the per-workgroup root counts of the numbering scan), rounded
 * up to 256 bytes.  0 for a bad dtype or shape, or a volume past the limit. */
size_t edt_hip_components_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
/* Refused before any device work, in this order: bad dtype, ndim outside 1..3, unused extents not 1 (EDT_ERR_BAD_ARG);
 * connectivity outside 1..ndim (EDT_ERR_BAD_ARG); a volume past the limit (EDT_ERR_UNSUPPORTED); NULL pointers, a missing
 * or too small workspace (EDT_ERR_BAD_ARG).  Enqueue-only on `stream`: no allocation, no synchronisation; the workspace is
 * initialised by the call itself (a reused one needs no memset).  d_out may not alias the labels.  d_n: one int64 on the
 * device.  An empty volume only sets *d_n = 0. */
int edt_hip_connected_components_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                        int connectivity, int binary, uint32_t *d_out, int64_t *d_n,
                                        void *d_workspace, size_t workspace_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels up once, out and n down once.  An empty volume sets *n = 0. */
int edt_hip_connected_components(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                 int connectivity, int binary, uint32_t *out, int64_t *n);

/* ---- fill holes: the enclosed cavities of a multi-label volume take the label of their wall ----------------------------
 * Conventions as in the connected-components section: x fastest, idx = x + sx * (y + sy * z), labels compared at full width
 * with the type's ==.
 * Background: a voxel whose label == 0.  -0.0 is background, NaN is foreground; for EDT_BOOL a zero byte is background.
 * Adjacency: connectivity = c, 1 <= c <= ndim, defined as in the connected-components section -- here it is the adjacency
 *   of the BACKGROUND (c = 1: the background is 2 * ndim-connected, scipy.ndimage.binary_fill_holes' default structure and
 *   fill_voids' rule).
 * Cavity: a connected component of background voxels, under c, none of whose voxels lies on the array's boundary --
 *   coordinate 0 or extent - 1 along any of the ndim axes.  A 3-D array with an axis of extent 1 therefore has no cavity.
 *   The cavities are what scipy.ndimage.binary_fill_holes(data != 0, generate_binary_structure(ndim, c)) fills.
 * Wall: the foreground voxels adjacent, under the same c, to a voxel of the cavity.  Never empty.
 * Representative: the wall voxel of smallest idx.
 * Fill: with binary != 0, or with EDT_BOOL, every cavity voxel takes the representative's label.  Otherwise a cavity is
 *   filled with the representative's label iff every wall voxel's label == it; a cavity whose wall holds two different
 *   labels is MIXED and stays 0, and so does one whose wall holds a NaN (which equals nothing).  Enclosed foreground is
 *   never touched: an island of label B inside label A is left alone.
 * Output: the labels' dtype, shape and memory order; foreground voxels and unfilled background are copied bit for bit.
 *   *n_filled (int64) is the number of voxels that changed from background to a label (a filled -0.0 voxel counts).
 * Determinism: the same call gives the same bytes.  Every reduction is an integer max or add; which thread wins an atomic
 *   never shows.
 * Limits: sx * sy * sz <= 2^31 - 1, as for connected components (32-bit parents, and the top bit of a root's word tags the
 *   state of its component).  Byte offsets are 64-bit. */

/* Scratch of edt_hip_fill_holes_device: 4 bytes per voxel (the parent plane of the background's union-find; a root's word
 * carries its component's state) plus the scratch of edt_hip_components_workspace_bytes, each rounded up to 256 bytes.
 * The mask labels == 0 is kept in the output array until the last sweep overwrites it.  0 for a bad dtype or shape, or a
 * volume past the limit. */
size_t edt_hip_fill_holes_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
/* Refused before any device work, in the order of edt_hip_connected_components_device and with its codes: bad dtype, ndim
 * outside 1..3, unused extents not 1 (EDT_ERR_BAD_ARG); connectivity outside 1..ndim (EDT_ERR_BAD_ARG); a volume past the
 * limit (EDT_ERR_UNSUPPORTED); NULL pointers, d_out == d_labels, a missing or too small workspace (EDT_ERR_BAD_ARG).
 * Enqueue-only on `stream`: no allocation, no synchronisation; the workspace is initialised by the call itself.  d_out: a
 * volume of the labels' dtype that does not overlap them.  d_n_filled: one int64 on the device.  An empty volume only sets
 * *d_n_filled = 0. */
int edt_hip_fill_holes_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity,
                              int binary, void *d_out, int64_t *d_n_filled, void *d_workspace, size_t workspace_bytes,
                              void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels up once, out and n_filled down once.  An empty volume sets
 * *n_filled = 0. */
int edt_hip_fill_holes(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                       void *out, int64_t *n_filled);

/* ---- dust: connected components are kept or removed by their voxel count ------------------------------------------------
 * Conventions as in the connected-components section: x fastest, idx = x + sx * (y + sy * z), labels compared at full width
 * with the type's ==; -0.0 is background; a NaN voxel is a component of its own, and joins its neighbours under binary;
 * EDT_BOOL is always binary.
 * Component: exactly a component of edt_hip_connected_components with the same connectivity and binary.  Its size is its
 *   voxel count.
 * Kept: a component is kept iff min_voxels <= size < max_voxels; with invert != 0 iff that does NOT hold.  max_voxels =
 *   INT64_MAX means "no upper bound" (min_voxels = t, max_voxels = INT64_MAX is cc3d.dust(threshold = t) and
 *   skimage.morphology.remove_small_objects(min_size = t)).
 * Output: the labels' dtype, shape and memory order.  A voxel of a kept component keeps its label bit for bit (a NaN its
 *   payload); a voxel of a removed component becomes all-zero bits; a background voxel is copied as it is (-0.0 keeps its
 *   sign).
 * Counts: three int64, in this order: components found, components kept, voxels removed.
 * Determinism: the same call gives the same bytes and counts.  Every reduction is an integer add; which thread wins an
 *   atomic never shows.
 * Limits: sx * sy * sz <= 2^31 - 1, as for connected components (32-bit parents; a root's word carries its component's size
 *   under the top bit).  Byte offsets are 64-bit. */

/* Voxels a wave of the size-counting kernel walks.  The wave sums what it meets of a component before it adds to the root's
 * word: a component costs it about one atomic add per span, however it is cut up (csrc/edt_dust.hip). */
#define EDT_HIP_DUST_COUNT_SPAN 8192

/* Scratch of edt_hip_dust_device: 4 bytes per voxel (the parent plane of the union-find; a root's own word carries its
 * component's size, there is no second plane) plus the scratch of edt_hip_components_workspace_bytes, each rounded up to 256
 * bytes -- what edt_hip_fill_holes_workspace_bytes gives.  0 for a bad dtype or shape, or a volume past the limit. */
size_t edt_hip_dust_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
/* Refused before any device work, in the order of edt_hip_connected_components_device and with its codes: bad dtype, ndim
 * outside 1..3, unused extents not 1 (EDT_ERR_BAD_ARG); connectivity outside 1..ndim (EDT_ERR_BAD_ARG); a volume past the
 * limit (EDT_ERR_UNSUPPORTED); then min_voxels < 0, max_voxels < min_voxels (EDT_ERR_BAD_ARG); NULL pointers, a missing or
 * too small workspace (EDT_ERR_BAD_ARG).  Enqueue-only on `stream`: no allocation, no synchronisation; the workspace is
 * initialised by the call itself.  d_out: a volume of the labels' dtype; d_out == d_labels is allowed (in place: the forest
 * is finished before the filter writes, and the filter's thread i reads and writes voxel i only); any other overlap is the
 * caller's error.  d_counts: three int64 on the device, zeroed on the stream by the call.  An empty volume only zeroes them. */
int edt_hip_dust_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity,
                        int binary, int64_t min_voxels, int64_t max_voxels, int invert, void *d_out, int64_t *d_counts,
                        void *d_workspace, size_t workspace_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels up once, out and the three counts down once.  out == labels is
 * allowed.  An empty volume zeroes counts[0..2]. */
int edt_hip_dust(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                 int64_t min_voxels, int64_t max_voxels, int invert, void *out, int64_t *counts);

/* ---- watershed: every label is split into the basins of a float32 field -------------------------------------------------
 * This is the STEEPEST-ASCENT watershed ("drop of water", hill climbing), stated as the connected components of a graph: no
 * iteration, no thread waits for another, the same bits on every run, nothing depends on who won an atomic.  It is NOT the
 * priority-flood watershed of skimage.segmentation.watershed: it takes no markers, and its boundaries follow the ascent rule
 * below, not a flooding order.  A voxel goes to its GREATEST neighbour, not along the steepest slope, so voxel sizes enter
 * through the field only.  min_saliency is ONE round of single-linkage merging, not the h-maxima hierarchy: a chain of shallow
 * saddles merges end to end.  Neither skimage nor cc3d is on the build machine: what is tested is this contract.
 * Conventions as in the connected-components section: x fastest, idx = x + sx * (y + sy * z); adjacency by connectivity = c,
 *   1 <= c <= ndim, as there.
 * Inputs: labels of any label dtype; field, one float32 per voxel; min_saliency = h, finite and >= 0, in the field's units.
 * Of one object: two neighbouring voxels are of one object iff connected_components would connect them: equal non-zero labels
 *   (-0.0 is background, a NaN voxel is alone), or, with binary != 0 or EDT_BOOL, both non-zero.
 * Field values: every comparison is an IEEE float32 comparison of the values as given; nothing is recomputed, squared or rounded.
 * Phase 1, ascent.  For a foreground voxel v let M be the greatest f(u) over its neighbours u of one object with v.  If
 *   M > f(v), v is joined to the neighbour that attains M -- on a tie the one of smallest idx.  Otherwise v is a TOP voxel and is
 *   joined to EVERY neighbour u of one object with f(u) == f(v).  The BASINS are the connected components of these joins.  A
 *   regional maximum, plateaus included, is one basin's summit.  A plateau that is not a maximum drains through its outlets;
 *   if it has outlets to two summits it joins their basins.
 * Phase 2, one round of saliency merges; skipped when h == 0, where it would change nothing.  peak(B) is the greatest f over
 *   basin B.  For every pair of neighbouring voxels u in A, v in B of one object, A and B basins of phase 1, A and B are joined
 *   iff  min(f(u), f(v)) >= min(peak(A), peak(B)) - h,  in float32 with one subtraction, on the phase-1 basins and their peaks.
 *   The result is the transitive closure of those joins; nothing that is evaluated depends on a join made.
 * Output: one uint32 per voxel -- 0 where the label is background, else the basin's number in 1..N, numbered as
 *   connected_components numbers: in ascending order of the smallest idx among a basin's voxels.  *n receives N as int64.
 *   With a constant field, or with h = 1e30 on a finite field, the output is that of connected_components bit for bit.
 * Field preconditions: +inf is legal (a transform without a black border produces it) and handled by IEEE alone.  A NaN on a
 *   foreground voxel is the caller's error: the partition is then unspecified, but the call terminates and writes numbers in
 *   0..N -- every loop is bounded by the forest's downhill rule, whatever the values.  The entry points do not look at the field.
 * Determinism: the same call gives the same output, bit for bit; the unions race, the result does not.
 * Limits: sx * sy * sz <= 2^31 - 1, as for connected components. */

/* Scratch of edt_hip_watershed_device: the output array serves as the parent plane; 4 bytes per voxel (the peak plane of
 * phase 2) plus the scratch of edt_hip_components_workspace_bytes, each rounded up to 256 bytes -- what
 * edt_hip_fill_holes_workspace_bytes gives.  0 for a bad dtype or shape, or a volume past the limit. */
size_t edt_hip_watershed_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
/* Refused before any device work, in the order of edt_hip_connected_components_device and with its codes: bad dtype, ndim
 * outside 1..3, unused extents not 1 (EDT_ERR_BAD_ARG); connectivity outside 1..ndim (EDT_ERR_BAD_ARG); a volume past the
 * limit (EDT_ERR_UNSUPPORTED); then min_saliency negative or not finite (EDT_ERR_BAD_ARG); NULL pointers, d_out overlapping
 * the labels or the field, a missing, too small or misaligned scratch (d_scratch is the call's workspace: 256-byte aligned, at
 * least the query's bytes) (EDT_ERR_BAD_ARG).  Enqueue-only on `stream`: no allocation, no synchronisation; the scratch is
 * initialised by the call itself.  d_n: one int64 on the device.  An empty volume only sets *d_n = 0. */
int edt_hip_watershed_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, const float *d_field,
                             int connectivity, int binary, float min_saliency, uint32_t *d_out, int64_t *d_n, void *d_scratch,
                             size_t scratch_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels (and the field) up once, out and n down once.  field == NULL: the
 * field is this library's own transform (with sqrt) of the labels -- of the mask labels != 0 under binary -- with the voxel
 * sizes wx, wy, wz and flags (EDT_FLAG_BLACK_BORDER or 0), computed on the device; with a field the voxel sizes and flags are
 * not looked at, except that any other flag is EDT_ERR_BAD_ARG, refused after min_saliency.  An empty volume sets *n = 0. */
int edt_hip_watershed(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, const float *field, float wx,
                      float wy, float wz, int flags, int connectivity, int binary, float min_saliency, uint32_t *out, int64_t *n);

/* ---- morphology: spherical erode / dilate / opening / closing of a label volume, through the distance transform ----------
 * Conventions as elsewhere in this header: x fastest, idx = x + sx * (y + sy * z); label 0 is background, compared with the
 * type's == (so -0.0 is background and a NaN is foreground); voxel sizes as for edt_hip_edtsq_device.  The structuring element is
 * the ball of physical radius `radius`: R2 = radius * radius, evaluated in fp64.  radius must be >= 0 with R2 finite -- NaN,
 * negative or overflowing values are EDT_ERR_BAD_ARG; only dilate accepts +inf, as expand_labels does.
 * The fields named below are exactly what edt_hip_edtsq_device writes (fp32, bit-identical to the reference); every comparison
 * is (double)field[p] > R2 or <= R2.  "Zero" means all-zero bits, "kept" means bit for bit.
 *
 * erode(labels, r, black_border, binary):  S = edtsq(labels, w, black_border) -- with binary, S = edtsq(m, w, black_border) for
 *   the uint8 mask m[p] = (labels[p] != 0).  out[p] = labels[p] if S[p] > R2, else zero (a -0.0 background voxel comes out
 *   +0.0).  r = 0 returns the labels otherwise unchanged.  EDT_BOOL is always the binary form.
 * dilate(labels, r):  exactly expand_labels(labels, r).
 * opening(labels, r, black_border, binary):  z[p] = 1 unless S[p] > R2, S as in erode, z uint8; B = edtsq(z, w, black border
 *   off); out[p] = labels[p] if B[p] <= R2, else zero.  If nothing survives the erosion B is +inf everywhere and out is zero.
 *   One binary transform serves every label at once: S[p] > R2 puts every voxel of another label farther than r from p, so
 *   no eroded voxel of another label lies within r of a voxel of label l, and the voxels within r of the eroded set, under
 *   their own labels, are the union over the labels of each label's opening.
 * closing(labels, r):  D = expand_labels(labels, r); m[p] = (D[p] != 0) as uint8; C = edtsq(m, w, black border off);
 *   out[p] = D[p] if labels[p] != 0 or C[p] > R2, else zero.  New voxels take the label expand_labels gives them, with its tie
 *   rule.  The labels[p] != 0 term makes closing extensive by construction, also for voxel sizes without a quantum, where
 *   expand_labels measures in fp64 and C is fp32.  Outside the volume counts as foreground for the erosion (border off). */
enum { EDT_MORPH_ERODE = 0, EDT_MORPH_DILATE = 1, EDT_MORPH_OPEN = 2, EDT_MORPH_CLOSE = 3 };
enum { EDT_MORPH_FARTHER = 0, EDT_MORPH_WITHIN = 1 };
#define EDT_FLAG_MORPH_BINARY 128   /* erode / opening: measure the mask labels != 0 */

/* The two streaming helpers the operations are composed from, on device-resident data.  Enqueue-only on `stream`: no
 * allocation, no synchronisation, no scratch.  Pointers as in "Alignment" above: any element offset is served; the vector
 * forms (four voxels per thread: 16 bytes of the field) are used where every pointer of the call has the alignment of four of
 * its elements, 16 bytes at the most; element by element otherwise, with the same bits.  Offsets are 64-bit (count may pass 2^32).  All seven label dtypes; 8-byte and float labels move as bit patterns. */
/* mask[i] = (labels[i] != 0) as one byte per voxel */
int edt_hip_is_foreground_device(const void *d_labels, int dtype, uint8_t *d_mask, int64_t count, void *stream);
/* pass(i) = rule == EDT_MORPH_FARTHER ? (double)field[i] > R2 : (double)field[i] <= R2   (EDT_MORPH_WITHIN);
 * d_guard != NULL: pass(i) |= guard[i] != 0   (guard has the dtype of values)
 * d_out   != NULL: out[i]  = pass ? values[i] : zero bits   (d_out == d_values allowed; d_values required)
 * d_mask  != NULL: mask[i] = pass ? 0 : 1
 * At least one of d_out / d_mask; a bad rule, a bad radius (+inf included), a bad dtype, count < 0 and missing pointers are
 * EDT_ERR_BAD_ARG before any device work. */
int edt_hip_morph_select_device(const void *d_values, const void *d_guard, int dtype, const float *d_field, double radius,
                                int rule, void *d_out, uint8_t *d_mask, int64_t count, void *stream);

/* Scratch of edt_hip_morphology_device, in this order, each part rounded up to 256 bytes: the fp32 field (4 bytes per voxel), the
 * uint8 mask (1 byte per voxel), then the scratch of the operation's transforms -- the largest any of its steps needs:
 * edt_hip_workspace_bytes_flags of EDT_U8, of the labels' dtype too where erode / opening measure the labels themselves, and
 * edt_hip_expand_labels_workspace_bytes for closing.  Dilate is expand_labels and needs only that scratch.  0 for a bad dtype,
 * shape or op, or flags the op does not take. */
size_t edt_hip_morphology_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int op, int flags);
/* The four operations on device-resident data, x fastest.  op: EDT_MORPH_*.  ndim in {1,2,3}, unused extents 1.  d_out has the
 * labels' dtype.  flags: EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY for erode / opening; 0 for dilate / closing.  Refused
 * before any device work, in this order: a bad dtype or shape, a bad op (EDT_ERR_BAD_ARG); a flag the op does not take
 * (EDT_ERR_UNSUPPORTED); a bad radius, bad voxel sizes; for a volume that is not empty NULL pointers, d_out == d_labels for
 * dilate and closing, a missing or too small workspace, a workspace that is not 256-byte aligned (EDT_ERR_BAD_ARG).
 * d_out == d_labels is allowed for erode and opening (in place: the last step reads and writes voxel i only, and the transforms
 * have finished with the labels); any other overlap is the caller's error.  Enqueue-only on `stream`: no allocation, no
 * synchronisation; the call initialises whatever it reads of its scratch (a reused workspace needs no memset).  An empty
 * volume is EDT_OK with nothing touched. */
int edt_hip_morphology_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                              float wz, int op, double radius, int flags, void *d_out, void *d_workspace, size_t workspace_bytes,
                              void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels up once, edt_hip_morphology_device, output down once.  Refusals as
 * above, in the same order; `output` may not overlap `labels` at all (EDT_ERR_BAD_ARG), for any op. */
int edt_hip_morphology(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                       int op, double radius, int flags, void *output);

/* ---- local thickness: for every voxel the radius of the largest ball of a ladder whose opening still contains it -------------
 * The granulometric ("porespy local_thickness", ImageJ "Local Thickness") thickness of every label at once, quantised to a
 * ladder of radii.  Conventions, labels, voxel sizes, black_border (EDT_FLAG_BLACK_BORDER) and binary (EDT_FLAG_MORPH_BINARY;
 * EDT_BOOL is always binary) as in "morphology" above; the fields are exactly what edt_hip_edtsq_device writes and every
 * comparison widens the fp32 field value to fp64.
 *
 * Radii r_1 < r_2 < ... < r_k, each finite and > 0 with r_j * r_j finite in fp64.
 *   S = edtsq(labels, w, black_border), or the field of the uint8 mask labels != 0 under binary: the field opening measures.
 *   For each j, O_j = { p : opening(labels, r_j, black_border, binary)[p] != 0 }, exactly as "morphology" defines opening:
 *     z_j[p] = 1 unless (double)S[p] > r_j^2;  B_j = edtsq(z_j, w, black border off);
 *     p in O_j  iff  p is foreground and (double)B_j[p] <= r_j^2.
 *   "Foreground" is (double)S[p] > 0, which is labels[p] != 0 under the type's own comparison (-0.0 is background, a NaN is
 *   foreground): a foreground voxel is at least one voxel away from anything that is not of its label.
 *   thickness[p] (fp32) = (float)r_j for the LARGEST j with p in O_j; +0.0 for background and for foreground voxels that lie in
 *   no O_j (thinner than the smallest ball).
 *   sizes[j] (int64) = |O_j|: the granulometry curve (cumulative size distribution).
 * "Largest j" is meant literally.  The openings by digital balls are not nested: a voxel may lie in O_j and not in O_(j-1), and
 * sizes need not be monotone.  The result is what overwriting in ascending order gives: T = 0; for j = 1..k: T[O_j] = r_j.
 *
 * The default ladder (radii == NULL): r_j = j * step in fp64, over all j >= 1 with r_j * r_j < Smax, where Smax is the largest
 * FINITE value of S widened to fp64, or 0 if S has none.  A ball with r^2 >= Smax erodes every voxel with a finite S.  The
 * Python layers pass step = the smallest |voxel size|.
 * One label everywhere and no black border: S = +inf everywhere.  The default ladder is then empty: thickness is zero and no radius
 * is used.  Explicit radii give thickness = (float)r_k everywhere and sizes[j] = voxels: no ball ever leaves the label.
 *
 * One step on device-resident fields.  Enqueue-only on `stream`: no allocation, no synchronisation, no scratch; pointers as in
 * "Alignment" above: any element offset is served, four voxels per thread where d_S, d_B and d_T are 16-byte and d_mask is 4-byte
 * aligned, one voxel per thread otherwise, with the same bits; offsets are 64-bit.
 *   d_B != NULL (a radius step): in(i) = (double)S[i] > 0 && (double)B[i] <= radius^2;  T[i] = (float)radius where in(i), and is
 *     left as it is elsewhere;  d_size != NULL: *d_size += the number of voxels with in(i).
 *   d_B == NULL (step 0; `radius` is ignored): T[i] = +0.0 for every i;  d_smax_bits != NULL: *d_smax_bits = max(*d_smax_bits, the
 *     bit pattern of the largest S[i] that is finite and >= 0) -- non-negative floats order as their bits.
 *   d_mask != NULL: mask[i] = (double)S[i] > next_radius^2 ? 0 : 1, the z of the next radius.  next_radius < 0 means none, and
 *     d_mask is given exactly when there is one.
 * The counters are accumulated into: the caller initialises them (zero) on the stream.  d_size belongs to a radius step,
 * d_smax_bits to step 0.  EDT_ERR_BAD_ARG before any device work: count < 0; d_S or d_T NULL; a radius (with d_B) or a next
 * radius >= 0 that is not finite and > 0 with a finite square, or NaN; d_mask without a next radius or a next radius without
 * d_mask; d_size without d_B; d_smax_bits with d_B.  count == 0 is EDT_OK once the arguments are through. */
int edt_hip_thickness_step_device(const float *d_S, const float *d_B, double radius, double next_radius, float *d_T,
                                  uint8_t *d_mask, int64_t *d_size, uint32_t *d_smax_bits, int64_t count, void *stream);

/* Scratch of edt_hip_local_thickness_device, in this order, each part rounded up to 256 bytes: S and B (fp32, 4 bytes per voxel
 * each), the uint8 mask (1 byte per voxel), the word of Smax, then the scratch of the transforms: edt_hip_workspace_bytes_flags
 * of EDT_U8, and of the labels' dtype where S is measured on the labels themselves.  0 for a bad dtype, shape or flags. */
size_t edt_hip_local_thickness_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags);
/* The whole operation on device-resident data, x fastest: S once, then per radius one binary transform and one step.
 * ndim in {1,2,3}, unused extents 1.  flags: EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY, anything else is EDT_ERR_UNSUPPORTED.
 * radii and n_used are HOST pointers; d_thickness (voxels floats) and d_sizes (int64) are on the device.
 * radii != NULL: n_radii >= 1 radii as above; `step` is ignored; d_sizes has n_radii entries; *n_used = n_radii.  The call is
 *   enqueue-only on `stream`: no allocation, no synchronisation, and it can be captured into a graph.
 * radii == NULL: the default ladder with `step` (finite, > 0, finite square).  The call SYNCHRONISES `stream` once, after the
 *   first transform, to read Smax back (4 bytes); a stream that is being captured is EDT_ERR_UNSUPPORTED before any device
 *   work.  n_radii (>= 0) is the room in d_sizes (d_sizes may be NULL if it is 0); *n_used = the ladder's length and
 *   d_sizes[0 .. *n_used) hold the sizes.  A ladder longer than n_radii is EDT_ERR_BAD_ARG after the first transform: *n_used
 *   then holds the length it needs and neither output holds a result.  r_j of that ladder is j * step.
 * d_sizes[0 .. n_radii) and the word of Smax are zeroed on the stream by kernels of the call (a replayed graph counts from
 * zero); the call initialises whatever it reads of its scratch (a reused workspace needs no memset).
 * Refused before any device work, in this order: a bad dtype or shape (EDT_ERR_BAD_ARG); flags (EDT_ERR_UNSUPPORTED); radii that
 * are not strictly ascending, not positive, not finite or whose square overflows, an explicit list with n_radii < 1, n_radii < 0,
 * a bad step for the default ladder; bad voxel sizes; for a volume that is not empty NULL pointers (d_labels, d_thickness,
 * n_used; d_sizes where it has entries), a missing or too small workspace, a workspace that is not 256-byte aligned
 * (EDT_ERR_BAD_ARG).  The outputs may not overlap the labels, the workspace or each other: the caller's error.  An empty volume
 * is EDT_OK with nothing touched. */
int edt_hip_local_thickness_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                                   float wz, int flags, const double *radii, int64_t n_radii, double step, float *d_thickness,
                                   int64_t *d_sizes, int64_t *n_used, void *d_workspace, size_t workspace_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels up once, edt_hip_local_thickness_device, thickness and
 * sizes[0 .. *n_used) down once.  Refusals as above, in the same order; thickness or sizes overlapping the labels or each other
 * is EDT_ERR_BAD_ARG.  After a ladder longer than n_radii nothing but *n_used is written. */
int edt_hip_local_thickness(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                            float wz, int flags, const double *radii, int64_t n_radii, double step, float *thickness,
                            int64_t *sizes, int64_t *n_used);

/* ---- medial axis: the integer medial axis of every label at once, a stencil on the feature transform ---------------------------
 * The method of Hesselink & Roerdink, "Euclidean skeletons of digital image and volume data in linear time by the integer medial
 * axis transform" (IEEE PAMI 30(12), 2008), in gather form: centre lines and centre surfaces of the objects of a label volume.
 * Conventions as in "feature transform": x fastest, idx = x + sx * (y + sy * z), label 0 is background, labels compared at full
 * width with their type's == (-0.0 is background, a NaN voxel equals nothing); voxel sizes as for edt_hip_edtsq_device.
 * F(p) is the feature of p from edt_hip_feature_transform_device with the same voxel sizes and border flag: the feature of the
 * labels themselves, or of the uint8 mask labels != 0 under EDT_FLAG_MORPH_BINARY (EDT_BOOL is always binary; a NaN is non-zero).
 *
 * A pair (p, q), q one of the 2 * ndim face neighbours of p INSIDE the volume, is eligible iff
 *   labels[p] != 0;  labels[q] == labels[p] under the type's own == (under binary: both non-zero);  and both voxels have a
 *   feature ("no feature" is every component -1 with the border off; with EDT_FLAG_BLACK_BORDER every voxel has one).
 * For an eligible pair, over the ndim axes c (the axes a call does not use contribute nothing):
 *   d_c = F(p)_c - F(q)_c   and   s_c = F(p)_c + F(q)_c - p_c - q_c   as 64-bit integers, then converted to fp64;
 *   A_c = (double)w_c * (double)w_c;
 *   sep  = (A_x (d_x d_x) + A_y (d_y d_y)) + A_z (d_z d_z)      the squared distance between the two features
 *   h    = (A_x (s_x s_x) + A_y (s_y s_y)) + A_z (s_z s_z)      four times the squared distance from the midpoint of p and q to
 *                                                               the midpoint of the features
 *   crit = (A_x (d_x s_x) + A_y (d_y s_y)) + A_z (d_z s_z)      which side of the features' bisector that midpoint lies on
 * in fp64, the product of the two integers first, then the product with A_c, then the sums in the order shown: every product and
 * sum rounded once, nothing contracted into an fma.
 * p is ON THE AXIS iff some eligible q has   sep > gamma * gamma   and   sep >= ratio * h   and   crit >= 0.
 *   gamma: constant pruning, a physical distance (the paper's test is gamma = 1 in voxel units: features more than one voxel apart);
 *   ratio = tan^2(theta / 2): angle pruning -- theta is the angle the two features subtend at the midpoint of p and q; 0 = off.
 * The two pruning tests are symmetric in (p, q) and crit is antisymmetric, bit for bit: of two neighbours whose features pass the
 * pruning, the one on whose side of the midpoint the bisector passes is on the axis -- both if it passes through the midpoint.
 * Every voxel decides for itself from what it reads (no atomics, no iteration): the same call gives the same output.
 * Where the voxel sizes share a quantum and the extents are small enough for every term to be an exact integer in fp64, the axis
 * is fully determined by the feature transform's tie rule; otherwise by the features the transform returned and by the evaluation
 * order above.
 * Output: out, of the labels' dtype: labels[p] bit for bit on the axis (a NaN keeps its payload), zero bits elsewhere.  Optionally
 * the radius function: radius[p] = field[p] on the axis and +0.0 elsewhere, for an fp32 field of the caller's choice. */

/* One step on device-resident data: d_features are the ndim planes edt_hip_feature_transform_device wrote for these labels (or
 * for their mask, under binary).  Enqueue-only on `stream`: no allocation, no synchronisation, no scratch.  Pointers as in
 * "Alignment" above: any element offset is served, by the same code (one element per lane).  Offsets are 64-bit.  All seven label
 * dtypes; 8-byte and float labels move as bit patterns.
 * flags: EDT_FLAG_BLACK_BORDER -- the border flag the features were computed with: it says which "no feature" convention
 *   applies -- and EDT_FLAG_MORPH_BINARY; anything else is EDT_ERR_UNSUPPORTED.
 * d_field and d_radius come both or neither.  d_out may not alias d_labels (the neighbours are still being read); any other
 * overlap is the caller's error.
 * EDT_ERR_BAD_ARG before any device work: a bad dtype, ndim or extent (unused extents 1); gamma or ratio NaN, negative or
 * infinite, or gamma * gamma not finite; bad voxel sizes; d_field without d_radius or d_radius without d_field; for a volume
 * that is not empty NULL d_labels, d_features or d_out, and d_out == d_labels.  A volume of more than 2^33 tiles of 62 x 4 x 16
 * voxels is EDT_ERR_UNSUPPORTED.  An empty volume is EDT_OK once the arguments are through. */
int edt_hip_medial_axis_step_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                                    float wz, const int32_t *d_features, int flags, double gamma, double ratio, void *d_out,
                                    const float *d_field, float *d_radius, void *stream);

/* Scratch of edt_hip_medial_axis_device, in this order, each part rounded up to 256 bytes: the ndim feature planes (int32, 4 bytes
 * per voxel each), the uint8 mask under binary (1 byte per voxel), the fp32 field with with_radius != 0 (4 bytes per voxel), then
 * the scratch of the transforms of what they read (the mask under binary, else the labels): edt_hip_feature_workspace_bytes, and
 * with_radius edt_hip_workspace_bytes_flags too, whichever is larger.  0 for a bad dtype, shape or flags. */
size_t edt_hip_medial_axis_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags, int with_radius);
/* The whole operation on device-resident data, x fastest: the mask (under binary), the feature transform, the field when
 * d_radius is wanted (not NULL: the workspace is then sized with with_radius = 1), and one step.
 * The field of d_radius is what edt_hip_edtsq_device with EDT_FLAG_SQRT writes for the same labels (under binary: for the mask),
 * voxel sizes and border: the distance to the nearest voxel of another label, the radius function.
 * ndim in {1,2,3}, unused extents 1.  flags: EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY, anything else is EDT_ERR_UNSUPPORTED.
 * d_out has the labels' dtype.  Refused before any device work, in this order: a bad dtype or shape (EDT_ERR_BAD_ARG); flags
 * (EDT_ERR_UNSUPPORTED); gamma or ratio as the step refuses them; bad voxel sizes; for a volume that is not empty NULL d_labels or
 * d_out, d_out == d_labels, a missing or too small workspace, a workspace that is not 256-byte aligned (EDT_ERR_BAD_ARG).  Any
 * other overlap is the caller's error.  Enqueue-only on `stream`: no allocation, no synchronisation; the call initialises
 * whatever it reads of its scratch (a reused workspace needs no memset).  An empty volume is EDT_OK with nothing touched. */
int edt_hip_medial_axis_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                               float wz, int flags, double gamma, double ratio, void *d_out, float *d_radius, void *d_workspace,
                               size_t workspace_bytes, void *stream);
/* The same on host buffers (synchronous, on the cached device buffers of the host-buffer entry points; under
 * edt_hip_set_devices on the first listed device): labels up once, edt_hip_medial_axis_device, out -- and radius if it is not
 * NULL -- down once.  Refusals as above, in the same order; out or radius overlapping the labels or each other is
 * EDT_ERR_BAD_ARG. */
int edt_hip_medial_axis(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                        int flags, double gamma, double ratio, void *out, float *radius);

#ifdef __cplusplus
}
#endif
#endif /* EDT_HIP_H */
