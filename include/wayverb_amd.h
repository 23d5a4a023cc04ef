/* wayverb_amd.h -- C ABI of the MI355X-native waveguide engine.
 *
 * Drop-in boundary for wayverb's `waveguide::run` hot path.  Every entry point below names
 * the reference interface it replaces (paths relative to the reference repository root).
 * The C++ mirror of `waveguide::run<pre,post>` (include/wayverb_amd/waveguide.h) and the
 * ctypes binding (wayverb_amd/engine.py) sit on top of exactly this ABI.
 *
 * Conventions
 *   - every function returns WV_OK (0) or a negative WV_E_* status; no exception crosses the ABI;
 *   - wv_last_error() returns the message for the calling thread's most recent failure;
 *   - plain pointers + sizes only; host pointers unless a parameter says "device";
 *   - node index = x + y*nx + z*nx*ny  (src/waveguide/src/cl/utils.cpp:33-36);
 *   - an engine handle is used from one thread at a time (as `run` is,
 *     src/waveguide/include/waveguide/waveguide.h:36-41).
 */
#ifndef WAYVERB_AMD_H
#define WAYVERB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------ */
enum {
    WV_OK = 0,
    WV_E_INVALID_ARGUMENT = -1,
    WV_E_INVALID_MESH = -2, /* node types / indices inconsistent with the data contract */
    WV_E_HIP = -3,          /* a HIP runtime call failed (message has the HIP error string) */
    WV_E_NO_DEVICE = -4,    /* no gfx950-class device visible: there is NO CPU fallback */
    WV_E_COMM = -5,         /* RCCL failure in the halo exchange */
    WV_E_STATE = -6         /* call not valid in the engine's current state */
};

/* ---- data contract: the reference's device structs, byte for byte -------------------------- */

/* boundary_type bits -- src/waveguide/include/waveguide/cl/utils.h:11-21 */
enum {
    WV_ID_NONE = 0,
    WV_ID_INSIDE = 1 << 0,
    WV_ID_NX = 1 << 1,
    WV_ID_PX = 1 << 2,
    WV_ID_NY = 1 << 3,
    WV_ID_PY = 1 << 4,
    WV_ID_NZ = 1 << 5,
    WV_ID_PZ = 1 << 6,
    WV_ID_REENTRANT = 1 << 7
};

/* error_code bits -- src/waveguide/include/waveguide/cl/structs.h:8-15 */
enum {
    WV_FLAG_SUCCESS = 0,
    WV_FLAG_INF = 1 << 0,
    WV_FLAG_NAN = 1 << 1,
    WV_FLAG_OUTSIDE_RANGE = 1 << 2,
    WV_FLAG_OUTSIDE_MESH = 1 << 3,
    WV_FLAG_SUSPICIOUS_BOUNDARY = 1 << 4
};

/* condensed_node -- cl/structs.h:19-22 (8 bytes) */
typedef struct wv_condensed_node {
    int32_t boundary_type;
    uint32_t boundary_index;
} wv_condensed_node;

/* coefficients_canonical -- cl/filter_structs.h:39-44,65-66 (112 bytes) */
typedef struct wv_coefficients_canonical {
    double b[7];
    double a[7];
} wv_coefficients_canonical;

/* boundary_data -- cl/structs.h:38-41 (56 bytes); boundary_data_array<D> is D of these */
typedef struct wv_boundary_data {
    double filter_memory[6];
    uint32_t coefficient_index;
    uint32_t reserved_;
} wv_boundary_data;

/* `waveguide::mesh` as `run` reads it (mesh.h:12-26, setup.h:27-48,
 * cl/boundary_index_array.h:8-11).  All arrays are borrowed for the duration of wv_create. */
typedef struct wv_mesh {
    int32_t nx, ny, nz;                            /* mesh_descriptor::dimensions */
    const wv_condensed_node* nodes;                /* [nx*ny*nz] */
    const wv_coefficients_canonical* coefficients; /* [num_coefficients] */
    uint32_t num_coefficients;
    const uint32_t* boundary_indices_1; /* [num_boundary_1][1] surface index per filter */
    const uint32_t* boundary_indices_2; /* [num_boundary_2][2] */
    const uint32_t* boundary_indices_3; /* [num_boundary_3][3] */
    uint64_t num_boundary_1, num_boundary_2, num_boundary_3;
} wv_mesh;

/* ---- engine options -------------------------------------------------------------------------- */
enum { WV_PRECISION_F32 = 0, /* pressures as the reference stores them (cl_float) */
       WV_PRECISION_F64 = 1  /* pressures in double: BASELINE.json north star */ };

typedef struct wv_tuning {
    int32_t pair;             /* two-step passes (pair_kernels.hip.h): -1 the engine decides by mesh size, 1 / 0 force on / off */
    int32_t pair_chunks;      /* workgroups along z of the march; 0 = fill whole rounds of workgroup slots */
    int32_t pair_inner_fix;   /* 1: 1-D boundary entries finish the inside node they face; 0: all such nodes go to the fix-up list */
    int32_t pair_wide;        /* 1: rows of more than 8 waves are shared by several workgroups; 0: such meshes keep single steps */
    int32_t pair_unit_waves;  /* sparse rooms: 1 = a listed unit runs only the live waves of its row */
    int32_t pair_unit_planes; /* sparse rooms: planes per work-list unit of the march (default 32) */
    int32_t pair_units_by_chunk; /* sparse rooms: 1 = an XCD takes its units chunk by chunk (neighbouring strips run together); 0 = strip by strip */
    int32_t tile_lists;       /* 1: rooms that leave much of the mesh outside visit live tiles / units only (see all_tiles) */
    int32_t fuse_pre_post;    /* 1: the next step's source / receiver work rides in this step's boundary launch where legal */
    int32_t graph;            /* 1: batches of single steps on small meshes are replayed as a hipGraph */
    int32_t boundary_lds;     /* 1: boundary workgroups stage the coefficient sets in LDS (<= 256 sets) */
    int32_t boundary_order;   /* 1: boundary entries processed in 64x8x8-brick order; 0: in the caller's order */
    int32_t boundary_xwall;   /* 1: in two- and three-step passes the wall nodes that face along x work on compact copies of what they would gather
                               * from the fields; 2: in two-step passes only (measurement); 0: nowhere */
    int32_t stream_ry, stream_nwx, stream_nwy, stream_zchunks; /* sweep tile shape as wv_set_stream_tuning; 0 = automatic */
    int32_t slab_early;       /* z-slabs, two-step passes: 1 = the faces AND the planes next to them are stepped ahead of the march, so that both
                               * halo exchanges of a pass (and the faces' second step, on the halo stream) run under it; 0 = the second exchange
                               * follows the march (the form of rounds 2 and 3); -1 (default) = 1 where a neighbour lives on another GPU (RCCL,
                               * or a slab of this process on another device), 0 between slabs that share a device.  Read once, at
                               * wv_create (the x-facing walls' compact copies leave out the planes an early pass steps ahead) */
    int32_t pair_split_rows;  /* 1: rows of 3..8 waves are marched as two overlapping windows (two smaller workgroups per CU); measurement only */
    int32_t fuse_planes;      /* z-slabs: 1 = the planes stepped around the halo exchanges take ONE launch (sweep + their boundary entries side by side) */
    int32_t whole_step;       /* single steps as ONE launch each (sweep workgroups and boundary workgroups side by side, the next step's source /
                               * receiver work served by the tiles that own those nodes): -1 the engine decides by mesh size (small meshes are
                               * bound by launches, not bytes), 1 / 0 force on / off.  Only where it is legal (one domain, the source and the
                               * receivers -- at most 63 -- on inside nodes); otherwise two launches per step as ever */
    int32_t triple;           /* three-step passes (triple_kernels.hip.h: 10.7 B per node-update where a two-step pass moves 16): -1 the engine
                               * decides by mesh size, 1 / 0 force on / off.  Wherever two-step passes run: one domain, a z-slab of a chain
                               * (three halo exchanges per pass; every rank's consent, like two-step passes), a room that leaves much of its
                               * mesh outside (a work list of live pieces).  A batch takes them wherever it has three steps left, then a
                               * two-step pass or a single step */
    int32_t triple_chunks;    /* workgroups along z of the three-step march; 0 = fill whole rounds of workgroup slots */
    int32_t triple_lanes;     /* bytes of a row per lane of the three-step march: 0 the engine decides (by row length, whichever ran faster on
                               * boxes of that size), 8 / 16 force */
} wv_tuning;

typedef struct wv_options {
    int32_t struct_size; /* = sizeof(wv_options); lets the struct grow */
    int32_t precision;   /* WV_PRECISION_* */
    int32_t device;      /* HIP device ordinal; -1 = the calling thread's current device */
    /* z-slab decomposition: plane z=0 (ghost_lo) / z=nz-1 (ghost_hi) of this mesh is a ghost
     * copy of the neighbouring rank's face plane; it is read, never updated, by this engine. */
    int32_t ghost_lo, ghost_hi;
    /* the error flag is brought to the host every `flag_interval` steps of wv_run
     * (1 = after every step, like waveguide.h:100-101; 0 = once per wv_run call) */
    int32_t flag_interval;
    int32_t stream_variant; /* 2 = plane sweep, y halos through LDS (default); kept for measurement:
                             * 3 = plane sweep without LDS, 0 = register z-march, 1 = naive */
    /* 0 (default): when a room leaves part of the mesh outside, the sweep visits only the tiles
     * that hold inside nodes (outside nodes are 0 and stay 0; wv_write_field / wv_write_value
     * re-enable the full sweep until they are 0 again).  1: always visit every tile. */
    int32_t all_tiles;
    /* 1: wv_mesh::nodes is a device pointer on `device` (what wv_scene_mesh_create_engine passes);
     * the boundary index and coefficient arrays are host arrays either way */
    int32_t nodes_on_device;
    /* z-slabs over RCCL: seconds a rank waits for a batch of steps (or for the ranks' agreement before one) before it gives up on
     * its peers -- WV_E_COMM, wv_last_error naming the rank, its neighbours and the stream that had not drained; the communicator
     * is aborted and the engine is good for wv_destroy only.  0 = 180 s, < 0 = wait for ever (plain hipStreamSynchronize). */
    int32_t comm_timeout_s;
    /* z-slabs, one rank per process (wv_comm_init): how the face planes reach the neighbouring ranks.
     *   WV_TRANSPORT_RCCL (default)  grouped ncclSend / ncclRecv on the halo stream;
     *   WV_TRANSPORT_IPC             copies into the neighbours' own fields, mapped with hipIpcOpenMemHandle (the handles travel
     *                                through the communicator at wv_comm_init; a copy engine moves the planes, no send / receive
     *                                kernel has to find CUs beside the march); the ranks' agreements and the flag OR stay on RCCL.
     *                                All ranks of a chain choose the same.  The engine then holds its four fields from wv_comm_init on. */
    int32_t transport;
    int32_t reserved_[5];
    /* HOW the engine does its work -- never what it computes: every setting gives bit-identical results
     * (tests/test_gpu_parity.py, test_gpu_pair.py run the golden cases under each).  wv_default_options
     * fills in the product's choices; the fields exist for measurement and for the tests.  The library
     * reads no environment variables (built with -DWV_DEBUG_ENV, WV_<FIELD> overrides a field: tools only). */
    wv_tuning tuning;
} wv_options;

enum { WV_TRANSPORT_RCCL = 0, WV_TRANSPORT_IPC = 1 };

typedef struct wv_engine wv_engine;

/* ---- life cycle ------------------------------------------------------------------------------ */

/* Replaces the set-up half of `run` (waveguide.h:43-76): zeroed previous/current fields, node,
 * coefficient and boundary-state buffers (get_boundary_data<N>, setup.h:68-85). */
int wv_create(const wv_mesh* mesh, const wv_options* options, wv_engine** out);
void wv_destroy(wv_engine* e);
const char* wv_last_error(void);
/* Fills `options` with defaults: F64 pressures (the default of every layer above this ABI too; F32 is
 * the reference's cl_float storage, bit for bit), the calling thread's current device, no ghosts,
 * flag_interval 0 (the flag words of a wv_run batch are read back once per batch; the step that
 * raised a flag is still reported exactly, see wv_run). */
void wv_default_options(wv_options* options);

/* ---- buffer access used by step pre/post-processors ----------------------------------------- */
enum { WV_BUF_CURRENT = 0, WV_BUF_PREVIOUS = 1 };

/* core::read_value / core::write_value on the pressure buffer
 * (src/core/include/core/cl/common.h:42-57); value converted to/from the engine precision. */
int wv_read_value(wv_engine* e, int buffer, uint64_t index, double* value);
int wv_write_value(wv_engine* e, int buffer, uint64_t index, double value);
/* core::read_from_buffer / cl::copy of the whole field (common.h:34-40;
 * preprocessor/gaussian.cpp:50).  elem_size 4 -> float[n], 8 -> double[n]. */
int wv_read_field(wv_engine* e, int buffer, void* dst, int elem_size);
int wv_write_field(wv_engine* e, int buffer, const void* src, int elem_size);
/* The same for planes [z_begin, z_begin + z_count) only: dst / src hold z_count*ny*nx elements.
 * (A 1024^3 field is 8.6 GB: a visualiser slice or a slab hand-over should not have to move it all.) */
int wv_read_planes(wv_engine* e, int buffer, int32_t z_begin, int32_t z_count, void* dst, int elem_size);
int wv_write_planes(wv_engine* e, int buffer, int32_t z_begin, int32_t z_count, const void* src, int elem_size);
/* Read back / restore boundary filter state in the reference layout boundary_data_array<D>[n_D]. */
int wv_read_boundary_data(wv_engine* e, int dimensionality, wv_boundary_data* dst);
int wv_write_boundary_data(wv_engine* e, int dimensionality, const wv_boundary_data* src);
/* mesh::set_coefficients (src/waveguide/src/setup.cpp:38-50): n must equal num_coefficients */
int wv_set_coefficients(wv_engine* e, const wv_coefficients_canonical* c, uint32_t n);
/* Page-locks `bytes` of the caller's host memory at `p` for the device (hipHostRegister) / releases it: reads and writes of fields,
 * planes and boundary data whose host side is registered memory go by DMA at the link's rate instead of through the runtime's staging
 * buffers (what cl_mirror.h does with the staging area of its cl::Buffer mirror).  Optional; WV_E_HIP when the runtime refuses. */
int wv_host_register(void* p, uint64_t bytes);
int wv_host_unregister(void* p);
/* Device addresses of the fields (element type per precision), for zero-copy wrappers.  Once a
 * pointer has been handed out the engine stops assuming that outside nodes hold zeros (see
 * wv_options::all_tiles) and keeps to one time step per pass over two fields, so that the pointers stay
 * the two fields (an engine that takes two-step passes rotates four). */
int wv_device_buffer(wv_engine* e, int buffer, void** device_ptr);

/* The state `run` carries from one loop iteration to the next (waveguide.h:80-123: `previous`, `current` and the boundary filter
 * memories), with the step count, the position in the source signal and the recorded receiver rows, copied aside ON THE DEVICE
 * (wv_checkpoint: two more fields of memory, allocated by the first call; WV_E_HIP when there is no room, the engine untouched) and
 * put back (wv_rollback: the engine continues from the checkpoint and, being deterministic, reproduces the abandoned steps bit for
 * bit).  For callers that run batches of steps ahead of per-step observers: `canonical`'s pressure callback may look at the field
 * of ANY step (canonical.h:66-69), so the C++ mirror runs batches speculatively and re-runs up to the step an observer looks at.
 * The source and the receivers must be the ones in place at the checkpoint (WV_E_STATE otherwise); wv_drop_checkpoint frees the copy.
 * One domain only: a slab of a chain (ghost planes, or a communicator of more than one rank) answers WV_E_STATE -- its neighbours'
 * planes and the transport's counters would have to go back with it. */
int wv_checkpoint(wv_engine* e);
int wv_rollback(wv_engine* e);
int wv_drop_checkpoint(wv_engine* e);

/* ---- stepping: the generic path ------------------------------------------------------------- */

/* One loop body of waveguide.h:82-119 without the callbacks: clear flag, launch the update
 * (previous <- next in place), read the flag back.  *flag receives the error_code bits. */
int wv_step(wv_engine* e, int32_t* flag);
/* std::swap(previous, current), waveguide.h:123 */
int wv_swap(wv_engine* e);

/* ---- stepping: the device-resident fast path ------------------------------------------------- */
enum { WV_SOURCE_NONE = 0,
       WV_SOURCE_HARD = 1, /* preprocessor::hard_source, preprocessor/hard_source.h:17-23 */
       WV_SOURCE_SOFT = 2  /* preprocessor::soft_source, preprocessor/soft_source.h:17-25 */ };

/* Signal injected at `node`, one sample per step, starting at the engine's current step. */
int wv_set_source(wv_engine* e, int kind, uint64_t node, const double* signal, uint64_t n);
/* Nodes whose pre-update `current` pressure is recorded every step
 * (postprocessor::node, src/postprocessor/node.cpp:14-18; the 7 reads of
 * directional_receiver.cpp:33-47).  node == UINT64_MAX records 0. */
int wv_set_receivers(wv_engine* e, const uint64_t* nodes, uint32_t n);
/* Run up to n_steps loop iterations on the device.  Stops early at the first step whose flag
 * is non-zero: *steps_done = completed steps (that step excluded), *flag = its error bits. */
int wv_run(wv_engine* e, uint64_t n_steps, uint64_t* steps_done, int32_t* flag);
/* Receiver samples of steps [first, first+n) as double[n][num_receivers]; steps driven by wv_step / wv_swap
 * record nothing (their rows are NaN). */
int wv_fetch_receivers(wv_engine* e, uint64_t first, uint64_t n, double* dst);
/* R directional receivers (postprocessor::directional_receiver, src/waveguide/src/postprocessor/directional_receiver.cpp:10-69)
 * recorded AND integrated on the device: one run of the mesh serves every listener in the room (the reference's application runs the
 * whole mesh once per source-receiver pair, src/combined/src/threaded_engine.cpp:155-162).  nodes[i] is the centre node of receiver
 * i; its six neighbours are compute_neighbors' (nx, px, ny, py, nz, pz).  Internally the 7 * n columns (per receiver the centre, then
 * ports 0..5) are recorded as wv_set_receivers records them; at the end of every batch of wv_run a kernel integrates them, one lane per
 * receiver, with the arithmetic of directional_receiver::operator() operation for operation, and only the {intensity, pressure}
 * records (16 B per receiver and step where the raw columns are 56) come to the host.  The records of n receivers are bit-identical
 * to those of n runs with one receiver each.
 *   - a centre with a neighbour off the grid: WV_E_INVALID_ARGUMENT, "Can't place directional_receiver at this node as it is adjacent
 *     to a boundary." (directional_receiver.cpp:21-27); the engine keeps what it had (everything is allocated before anything changes)
 *   - records of completed steps are always fetchable; after a run that stopped on a flag the velocities are as meaningless as the fields
 *   - steps taken by wv_step / wv_swap record NaN rows and leave the velocities alone
 *   - wv_checkpoint copies the velocities and the log's length aside, wv_rollback puts both back
 *   - wv_set_receivers, or wv_set_directional_receivers(e, NULL, 0, ...), leaves the mode; in it wv_fetch_receivers answers WV_E_STATE
 *     (and wv_fetch_directional answers WV_E_STATE outside it)
 *   - a slab of a chain (ghost planes, or a communicator of more than one rank) answers WV_E_STATE: a receiver next to a cut has a
 *     neighbour in a ghost plane, and nothing pins the reading of ghost planes by receivers in every form of pass.  Chains record the
 *     7 * n columns with wv_set_receivers and integrate them with wv_directional_accumulate (below): the same records, bit for bit.
 * wv_fetch_directional: records of steps [first, first + n) as wv_directional_output[n][R] (the struct is declared with the host-side
 * post-processing below). */
struct wv_directional_output;
int wv_set_directional_receivers(wv_engine* e, const uint64_t* nodes, uint32_t n, double spacing, double sample_rate,
                                 double ambient_density);
int wv_fetch_directional(wv_engine* e, uint64_t first, uint64_t n, struct wv_directional_output* dst /* [n][R] */);
/* Number of loop iterations completed since creation. */
int wv_step_count(wv_engine* e, uint64_t* steps);

/* ---- field snapshots while a run keeps going --------------------------------------------------- */
/* The reference's application hangs a mesh-pressure visualiser off the per-step callback (src/combined/src/engine.cpp:158-169): it
 * looks at the field while `run` goes on.  Here the field never leaves the device during wv_run, and reading it (wv_read_planes)
 * between short runs stops the compute stream for an allocation, a packing launch and a copy.  A snapshot plan has the engine record
 * the field itself: a box of the mesh, every s-th node along each axis, every `period` steps, as floats (a double rounds to nearest,
 * exactly as wv_read_planes with elem_size 4 converts), captured ON THE DEVICE directly behind the pass that produced the step and
 * copied to page-locked host memory on a stream of its own while the next steps already run.
 *
 * The snapshot "of step s" is the field after exactly s completed steps: bit for bit the floats wv_read_planes(e, WV_BUF_CURRENT, ...,
 * 4) returns when wv_step_count says s, subsampled to the box -- what `post` (and `canonical`'s callback) sees at step s, but for the
 * source's sample of step s, which the loop puts into its node before `post` looks and after the snapshot is taken.  Steps
 * count from the engine's creation; step first_step + j * period is captured if it is >= the step count when the plan was set (a
 * step equal to that count: at the start of the next wv_run).  Snapshots are numbered 0, 1, ... in the order taken since the plan
 * was set; the host holds the last `keep` of them (0: all).
 *
 *   - a run that stops on a flag at step f holds no snapshot of a step > f
 *   - wv_rollback drops the snapshots of steps after the checkpoint; the re-run takes them again, bit-identical
 *   - wv_step / wv_swap take no snapshots (as they record no receiver rows); snapshot steps they pass are passed
 *   - on return from wv_run every snapshot of a completed step can be fetched
 *   - passes end on snapshot steps (a two- or three-step pass never holds the steps inside it as whole fields) and a batch of steps
 *     holds no more captures than the ring has slots, so a short period costs some of the passes' advantage; results are
 *     bit-identical with and without a plan
 *
 * wv_set_snapshots allocates the device ring and its page-locked twin (WV_E_HIP when there is no room, the engine and any earlier
 * plan untouched); a new plan replaces the old one and forgets what it held; NULL stops recording, forgets and frees (as does
 * wv_destroy).  WV_E_INVALID_ARGUMENT for a box that leaves the mesh, a zero stride or a zero period.  One domain only: a slab of a
 * chain (ghost planes, or a communicator of more than one rank) answers WV_E_STATE -- every rank would hold a part of the box and
 * the chain would have to agree on the cuts; nobody needs that yet.
 * wv_fetch_snapshots: snapshots [first, first + n) as float[n][nz][ny][nx], their steps in steps[n] (may be NULL);
 * WV_E_INVALID_ARGUMENT for one that was dropped or is not taken yet.  wv_snapshot_count: *taken = snapshots taken since the plan
 * was set, *first_held = the oldest still held (either may be NULL). */
typedef struct wv_snapshot_plan {
    int32_t x0, y0, z0;  /* first node of the box */
    int32_t nx, ny, nz;  /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;  /* take every s-th node along the axis, >= 1 */
    uint64_t first_step; /* snapshots at first_step + j * period, j = 0, 1, ... */
    uint64_t period;     /* >= 1 */
    uint32_t keep;       /* snapshots held on the host; older ones are dropped.  0 = all */
    uint32_t reserved;
} wv_snapshot_plan;
int wv_set_snapshots(wv_engine* e, const wv_snapshot_plan* plan);
int wv_snapshot_count(wv_engine* e, uint64_t* taken, uint64_t* first_held);
int wv_fetch_snapshots(wv_engine* e, uint64_t first, uint64_t n, float* dst /* [n][nz][ny][nx] */, uint64_t* steps /* [n] */);

/* ---- field spectra: a box of the field Fourier-transformed on the device ------------------------- */
/* What the room does at a given frequency everywhere at once -- mode shapes, steady-state pressure maps, the transfer function from
 * the source to every node of a plane -- is the Fourier transform over time of a box of the field.  With snapshots alone every
 * capture crosses the link and the host array grows with the run; a spectrum plan has the engine capture the box as a snapshot
 * plan would (the same box / stride semantics, the same cadence) and accumulate, per node taken and per frequency, a running
 * discrete Fourier sum ON THE DEVICE.  Nothing crosses the link until the caller fetches the K complex fields.
 *
 * Definition.  p_j is the float a snapshot of plan step n_j holds for the node: the field after exactly n_j completed steps, a
 * double rounded to nearest (the snapshot block above, unchanged).  f_k is in cycles per step, 0 <= f_k <= 0.5.  The twiddles come
 * from one exported function, which the engine itself uses on the host (the device evaluates no trigonometric function):
 *     wv_spectrum_twiddle(f, step, &c, &s):   x = f * (double)step;  x -= floor(x);  c = cos(2 pi x);  s = sin(2 pi x)   (libm, double)
 * and the sums run in capture order j = 0, 1, ..., in double, the product rounded, then the sum rounded:
 *     re[k] = re[k] + (double)p_j * c(j, k)          im[k] = im[k] - (double)p_j * s(j, k)
 * so X_k = sum_j p_j e^(-2 pi i f_k n_j), and a loop over the snapshots in the same order that evaluates `a + p * c` on float64
 * arrays reproduces the sums BIT FOR BIT.  No window is applied: a caller who wants one changes the cadence or post-processes.
 *
 *   - 1 <= n_freqs <= 64; a frequency outside [0, 0.5], a NaN, a box that leaves the mesh, a zero stride or a zero period:
 *     WV_E_INVALID_ARGUMENT
 *   - everything (the stage of 16 captures, 64 bytes per node; the sums, 16 n_freqs bytes per node) is allocated when the plan is
 *     set: with no room the call answers WV_E_HIP and leaves the engine and any earlier plan untouched.  A new plan replaces the old
 *     one and forgets its sums; a NULL plan stops, forgets and frees (as does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE (the snapshot plan's reason)
 *   - a spectrum plan and a snapshot plan are EXCLUSIVE: both decide where passes end; setting one while the other is active answers
 *     WV_E_STATE
 *   - after a run that stopped on a flag at step f (an overflow, or keep_going cleared) the sums hold exactly the captures of steps
 *     <= f, and wv_spectrum_count says how many: a capture of a step that was never committed is never folded in
 *   - wv_step / wv_swap capture nothing; plan steps they pass are passed, as for snapshots
 *   - wv_checkpoint copies the sums and the count aside (the copy is allocated by the first checkpoint taken under a plan: WV_E_HIP,
 *     engine untouched, when there is no room); wv_rollback puts both back, and the re-run reproduces them bitwise.  A plan set
 *     AFTER the checkpoint makes wv_rollback answer WV_E_STATE, as a changed source does
 *   - wv_fetch_spectrum may be called any time outside wv_run; it folds what is staged and leaves the plan running, so fetching
 *     twice during a long run gives two consistent partial sums
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * wv_spectrum_count: *captures = captures of completed steps since the plan was set, *last_step = the step of the last of them
 * (either may be NULL).  wv_fetch_spectrum: the sums as complex128 [n_freqs][nz][ny][nx] (re, im interleaved), *captures (may be
 * NULL) = how many captures they hold. */
typedef struct wv_spectrum_plan {
    int32_t x0, y0, z0;  /* first node of the box */
    int32_t nx, ny, nz;  /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;  /* take every s-th node along the axis, >= 1 */
    uint64_t first_step; /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;     /* >= 1 */
    uint32_t n_freqs;    /* K, 1 .. 64 */
    uint32_t reserved;
} wv_spectrum_plan;
int wv_set_spectrum(wv_engine* e, const wv_spectrum_plan* plan, const double* cycles_per_step /* [n_freqs] */);
int wv_spectrum_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_spectrum(wv_engine* e, double* dst /* [n_freqs][nz][ny][nx][2]: complex128 */, uint64_t* captures);
void wv_spectrum_twiddle(double cycles_per_step, uint64_t step, double* c, double* s);

/* ---- energy decay maps: time-binned field energy folded on the device -------------------------- */
/* How long sound lingers, and where -- the energy decay curve and the reverberation times (EDT, T20, T30) at every node of an
 * audience plane, the level map under broadband excitation -- follows from the squared field summed over time.  The reference
 * computes it for one receiver trace at a time (src/core/include/core/schroeder.h).  With snapshots alone every capture crosses the
 * link and the host array grows with the run; a decay plan has the engine capture the box as a snapshot plan would (the same box /
 * stride semantics, the same cadence) and accumulate, per node taken, the energy of the captures in n_bins TIME BINS ON THE DEVICE.
 * Nothing crosses the link until the caller fetches the n_bins doubles per node.  The backward sums of the bins are the Schroeder
 * integral exactly at the bin edges (only the order of summation differs from the per-sample curve): wayverb_amd/decay.py derives
 * the decay curve and the decay times from them with the reference's own regression.
 *
 * Definition.  p_j is the float a snapshot of plan step n_j holds for the node: the field after exactly n_j completed steps, a
 * double rounded to nearest (the snapshot block above, unchanged).  Capture j counts the committed captures since the plan was set
 * (0, 1, ...) and goes to bin
 *     b(j) = min(j / bin_captures, n_bins - 1)                      (integer division)
 * so every bin holds bin_captures captures but the last, which is open-ended: the backward sums stay exact tail sums at every
 * earlier edge however long the run.  The sums start at +0.0 and run in capture order, in double:
 *     E[b(j)] = E[b(j)] + (double)p_j * (double)p_j
 * The product of two converted floats is exact in double; the one rounding per capture is the sum's.  A loop over the snapshots of
 * the same plan that evaluates `E[b] = E[b] + p * p` on float64 arrays therefore reproduces the bins BIT FOR BIT.
 *
 *   - 1 <= n_bins <= 4096 and bin_captures >= 1; otherwise, and for a box that leaves the mesh, a zero stride or a zero period:
 *     WV_E_INVALID_ARGUMENT
 *   - everything (the stage of 16 captures, 64 bytes per node; the bins, 8 n_bins bytes per node; two tables of 16 bin indices) is
 *     allocated when the plan is set: with no room the call answers WV_E_HIP and leaves the engine and any earlier plan untouched.
 *     A new plan replaces the old one and forgets its bins; a NULL plan stops, forgets and frees (as does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE (the snapshot plan's reason), and wv_run_group refuses an engine with a
 *     plan, as it does for the other plans
 *   - a decay plan, a spectrum plan and a snapshot plan are EXCLUSIVE: each decides where passes end.  Each of the three setters
 *     answers WV_E_STATE while another plan is active, and wv_last_error names the plan to stop
 *   - after a run that stopped on a flag at step f (an overflow, or keep_going cleared) the bins hold exactly the captures of steps
 *     <= f, and wv_decay_count says how many: a capture of a step that was never committed is never folded in
 *   - wv_step / wv_swap capture nothing; plan steps they pass are passed, as for snapshots
 *   - wv_checkpoint folds what is staged and copies the bins, the capture count and the next plan step aside (the copy is allocated
 *     by the first checkpoint taken under a plan: WV_E_HIP, engine untouched, when there is no room); wv_rollback puts them back,
 *     and the re-run reproduces the bins bitwise.  A plan set AFTER the checkpoint makes wv_rollback answer WV_E_STATE
 *   - wv_fetch_decay may be called any time outside wv_run; it folds what is staged and leaves the plan running, so fetching
 *     twice during a long run gives two consistent partial sums
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * wv_decay_count: *captures = captures of completed steps since the plan was set, *last_step = the step of the last of them
 * (either may be NULL).  wv_fetch_decay: the bins as float64 [n_bins][nz][ny][nx], *captures (may be NULL) = how many captures
 * they hold. */
typedef struct wv_decay_plan {
    int32_t x0, y0, z0;    /* first node of the box */
    int32_t nx, ny, nz;    /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;    /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;   /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;       /* >= 1 */
    uint32_t n_bins;       /* 1 .. 4096 */
    uint32_t bin_captures; /* W >= 1: captures per bin (the last bin is open-ended) */
} wv_decay_plan;
int wv_set_decay(wv_engine* e, const wv_decay_plan* plan);
int wv_decay_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_decay(wv_engine* e, double* dst /* [n_bins][nz][ny][nx] */, uint64_t* captures);

/* ---- band-limited decay maps: octave-band filters ahead of the energy fold ---------------------- */
/* Reverberation times are quoted per octave band (ISO 3382), and an impulse-driven rectilinear mesh carries energy up to Nyquist
 * while the waveguide is trusted below about a quarter of the sample rate: the broadband bins above sum both.  wv_set_decay_bands is
 * a decay plan with a FILTER BANK in front of the square: n_bands cascades of n_sections biquad sections, run per node on the device
 * on the series of captures, each band with bins of its own.  wv_decay_plan is the plan above, unchanged, and so is wv_set_decay.
 * The arithmetic is the reference's core::filter::biquad / series_biquads<N> (src/core/include/core/filters_common.h), a wv_biquad
 * its biquad::coefficients (a0 == 1); wv_butterworth_bandpass and wv_bandpass_biquad restate its designs.
 *
 * Definition.  p_j is the snapshot float of committed capture j (the block above) and x = (double)p_j.  For band k the sections
 * s = 0 .. n_sections - 1 run in series on the node's own state z1[k][s], z2[k][s], which starts at +0.0; every product and sum is
 * rounded on its own, nothing is contracted, in exactly this association:
 *     out = x * b0 + z1
 *     z1  = (x * b1 - a1 * out) + z2
 *     z2  = x * b2 - a2 * out
 *     x   = out                                                     (into the next section)
 * and with y = x after the last section
 *     E[k][b(j)] = E[k][b(j)] + y * y                               (the product is rounded, then the sum)
 * b(j) is the plain plan's bin.  A loop over the snapshots of the same plan that evaluates these lines on float64 arrays
 * (wayverb_amd/decay.py: banded_bins) reproduces bins AND states BIT FOR BIT; wv_biquad_run is the same cascade on the host.
 *
 *   - 1 <= n_bands <= 8, 1 <= n_sections <= 4, every coefficient finite; otherwise, and for whatever wv_set_decay refuses in a
 *     plan: WV_E_INVALID_ARGUMENT.  A NULL plan stops, forgets and frees the plan, as wv_set_decay(e, NULL) does (either call
 *     stops either kind)
 *   - everything is allocated when the plan is set: the stage (64 bytes per node), 8 n_bins n_bands bytes of bins and
 *     16 n_sections n_bands bytes of filter state per node, the coefficient table and the two bin tables.  With no room the call
 *     answers WV_E_HIP and leaves the engine and any earlier plan untouched
 *   - box, stride, cadence, one domain only, wv_run_group's refusal, wv_step / wv_swap capturing nothing, fetching any time
 *     outside wv_run, and bit-identical fields / receiver rows / flags are the plain plan's rules.  A banded plan IS a decay plan
 *     where plans exclude each other: the snapshot and spectrum setters refuse while it is active and it refuses while they are,
 *     and the two kinds of decay plan refuse each other too; wv_last_error names the plan to stop
 *   - after a run that stopped on a flag at step f the bins hold exactly the captures of steps <= f, and the filter states have
 *     seen exactly those: a continued run goes on as if the dropped captures had never been taken
 *   - wv_checkpoint copies bins AND filter states aside and wv_rollback puts both back; the re-run is bitwise the same
 *   - wv_decay_count and the queries WV_QUERY_DECAY_CAPTURES / _FOLDS / _NS serve both kinds of plan.  wv_fetch_decay under a
 *     banded plan answers WV_E_STATE, and so does wv_fetch_decay_bands under a plain plan; wv_last_error names the other call
 *
 * What the caller owns.  The series the filters see is sampled at sample_rate / period: design the sections for THAT rate.  With
 * period > 1 field content above sample_rate / (2 period) aliases into the bands, so an impulse source needs period = 1 -- which
 * ends every pass on every step -- while a source band-limited below sample_rate / 6 can run at period = 3 and keep three-step
 * passes.  Plan steps skipped by wv_step / wv_swap are gaps in the series.
 *
 * Host side, no GPU.  wv_biquad_run filters in[0 .. n) through the cascade into out (which may be `in`); state [n_sections][2]
 * = z1, z2 per section is read and written back, NULL = start from +0.0 and discard.  wv_butterworth_bandpass writes the two
 * sections of compute_hipass_butterworth_coefficients<2>(lo_hz) followed by the two of compute_lopass_butterworth_coefficients<2>
 * (hi_hz): a 4th-order Butterworth slope on either side.  wv_bandpass_biquad is compute_bandpass_biquad_coefficients.  Both want
 * 0 < lo_hz < hi_hz < sample_rate / 2 (WV_E_INVALID_ARGUMENT otherwise) and keep the reference's order of operations. */
typedef struct wv_biquad { double b0, b1, b2, a1, a2; } wv_biquad;   /* 40 bytes; core::filter::biquad::coefficients, a0 == 1 */
int wv_set_decay_bands(wv_engine* e, const wv_decay_plan* plan,
                       const wv_biquad* sections /* [n_bands][n_sections] */, uint32_t n_bands, uint32_t n_sections);
int wv_fetch_decay_bands(wv_engine* e, double* dst /* [n_bands][n_bins][nz][ny][nx] */, uint64_t* captures);
int wv_biquad_run(const wv_biquad* sections, uint32_t n_sections, const double* in, uint64_t n,
                  double* state /* [n_sections][2] in/out, or NULL */, double* out);
int wv_butterworth_bandpass(double lo_hz, double hi_hz, double sample_rate, wv_biquad out[4]);
int wv_bandpass_biquad(double lo_hz, double hi_hz, double sample_rate, wv_biquad* out);

/* ---- intensity maps: time-binned sound intensity of a box, on the device ----------------------- */
/* Snapshots, spectra and decay maps see pressure and nothing else.  Where the energy COMES FROM and where it goes -- the direction
 * the early energy reaches a seat from, the wall that sends the late echo, how diffuse the field is over an audience plane -- is
 * answered by the sound intensity vector I = p v.  The reference computes it for one node at a time
 * (postprocessor::directional_receiver, src/waveguide/src/postprocessor/directional_receiver.cpp:29-69) and
 * wv_set_directional_receivers does so for a list of nodes, a 16-byte record per receiver and step.  An intensity plan has the
 * engine capture a box as a decay plan would and accumulate, per node taken, the three components of I AND the squared pressure in
 * n_bins time bins on the device: 32 n_bins bytes per node cross the link when the caller asks, however long the run.
 *
 * wv_intensity_plan holds wv_decay_plan's fields with the same meaning, and `spacing, sample_rate, ambient_density`: the three
 * arguments of the reference's directional_receiver constructor.
 *
 * Definition.  For every node taken (c its index, n_i its six neighbours) and every committed capture j, in capture order:
 *     pressure       = (float) field[c]                                  the snapshot float of a snapshot plan, unchanged
 *     surrounding[i] = (float)( (double)( (float)field[n_i] - pressure ) / spacing )      i = 0..5: ports nx, px, ny, py, nz, pz
 *     gx = surrounding[1] - surrounding[0]                               (float; gy from ports 3, 2 and gz from 5, 4 likewise)
 *     m  = (double)g * 0.5
 *     v  = v - m / k                                                     k = ambient_density * sample_rate; v is double[3] per
 *                                                                        node and starts at +0.0; the division is IEEE
 *     I[a][b(j)] = I[a][b(j)] + v[a] * (double)pressure                  a = x, y, z (the product is rounded, then the sum)
 *     E[b(j)]    = E[b(j)]    + (double)pressure * (double)pressure
 * b(j) = min(j / bin_captures, n_bins - 1) is the decay plan's bin, the last bin open-ended.  The first lines are the directional
 * receivers' (wv_directional_accumulate): the same casts, the same association; nothing is contracted.  A capture "of step s" is a
 * snapshot's, for the centre and all six neighbours: the field after exactly s completed steps, before the loop puts the source's
 * sample of step s into its node.  E is therefore, bit for bit, what a plain decay plan of the same box and cadence holds, and a
 * NumPy loop over snapshots of the box's hull that evaluates these lines (wayverb_amd/intensity.py: intensity_bins; the float
 * lines on float32 arrays, the rest on float64) reproduces I, E AND the velocities BIT FOR BIT.
 *
 *   - 1 <= n_bins <= 4096, bin_captures >= 1, strides and period >= 1, and spacing, sample_rate, ambient_density positive and
 *     finite; otherwise, and for a box that leaves the mesh: WV_E_INVALID_ARGUMENT
 *   - a taken node with a neighbour off the grid answers WV_E_INVALID_ARGUMENT with the reference's sentence, as
 *     wv_set_directional_receivers does: x0 >= 1 and x0 + (nx - 1) sx <= mesh_nx - 2, likewise for y and z.  Neighbours inside a
 *     wall are read as the field holds them: the reference refuses only an off-grid neighbour
 *   - everything (the stage of 16 captures, 256 bytes per node; the bins, 32 n_bins bytes per node; the velocities, 24 bytes per
 *     node; two tables of 16 bin indices) is allocated when the plan is set: with no room the call answers WV_E_HIP and leaves the
 *     engine and any earlier plan untouched.  A new plan replaces the old one and forgets its sums; a NULL plan stops, forgets and
 *     frees (as does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE, and wv_run_group refuses an engine with a plan
 *   - an intensity plan excludes every other plan (snapshot, spectrum, both kinds of decay, arrival, lateral): every setter answers
 *     WV_E_STATE while another plan is active, and wv_last_error names the plan to stop
 *   - after a run that stopped on a flag at step f, bins AND velocities have seen exactly the captures of steps <= f: a continued
 *     run goes on as if the dropped captures had never been taken
 *   - wv_step / wv_swap capture nothing; the plan steps they pass are gaps in the series the integrator sees
 *   - wv_checkpoint folds what is staged and copies bins, velocities, the capture count and the next plan step aside (the copies are
 *     allocated by the first checkpoint taken under a plan: WV_E_HIP, engine untouched, when there is no room); wv_rollback puts
 *     them back, and the re-run is bitwise the same.  A plan set AFTER the checkpoint makes wv_rollback answer WV_E_STATE
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * What the caller owns.  The integrator sees a series sampled at sample_rate / period: pass THAT rate.  With period > 1 field
 * content above sample_rate / (2 period) aliases, so an impulse source needs period = 1 -- which ends every pass on every step --
 * while a source band-limited below sample_rate / 6 can run at period = 3 and keep three-step passes (the decay plan's argument).
 *
 * wv_intensity_count: as wv_decay_count.  wv_fetch_intensity: float64 [4][n_bins][nz][ny][nx] = Ix, Iy, Iz, E; *captures (may be
 * NULL) = how many captures they hold.  It may be called any time outside wv_run, folds what is staged and leaves the plan running.
 * wv_fetch_intensity_velocity: the carried velocities, float64 [3][nz][ny][nx], after the same fold.
 * wv_fetch_directional_velocity: the directional receivers' carried velocities, float64 [n][3] (the same integrator's state on the
 * other path; WV_E_STATE without directional receivers). */
typedef struct wv_intensity_plan {
    int32_t x0, y0, z0;    /* first node of the box */
    int32_t nx, ny, nz;    /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;    /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;   /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;       /* >= 1 */
    uint32_t n_bins;       /* 1 .. 4096 */
    uint32_t bin_captures; /* W >= 1: captures per bin (the last bin is open-ended) */
    double spacing;        /* mesh_descriptor::spacing, > 0 */
    double sample_rate;    /* of the CAPTURED series: the mesh's sample rate / period, > 0 */
    double ambient_density;/* > 0 */
} wv_intensity_plan;
int wv_set_intensity(wv_engine* e, const wv_intensity_plan* plan);
int wv_intensity_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_intensity(wv_engine* e, double* dst /* [4][n_bins][nz][ny][nx]: Ix, Iy, Iz, E */, uint64_t* captures);
int wv_fetch_intensity_velocity(wv_engine* e, double* dst /* [3][nz][ny][nx] */);
int wv_fetch_directional_velocity(wv_engine* e, double* dst /* [n][3] */);

/* ---- arrival-aligned energy maps: onset, peak and energy binned from each node's own arrival ---- */
/* Decay and intensity maps bin every node by ONE clock: the capture's number since the plan was set.  Clarity C50 / C80, definition
 * D50 and centre time Ts (ISO 3382) measure early and late energy from the arrival of the direct sound AT THAT SEAT, and across a
 * hall the direct sound arrives tens of milliseconds apart -- the size of the 50 / 80 ms windows themselves.  An arrival plan has
 * the engine capture a box exactly as a decay plan captures it and keep, per node taken and on the device: the capture at which the
 * node's direct sound arrived (its onset), the node's peak and when it occurred, the squared pressure summed into bins counted from
 * the node's OWN onset, the energy ahead of the onset, and the first time moment of the energy behind it.  What crosses the link is
 * 28 + 8 n_bins bytes per node when the caller asks, however long the run; wayverb_amd/arrival.py turns it into arrival time, direct
 * level, C50 / C80, D50 and Ts.
 *
 * Definition.  p_c is the float a snapshot of the same plan holds for the node (the snapshot block above, unchanged); c = 0, 1, ...
 * counts the committed captures since the plan was set.  thr is the node's threshold: the plan's scalar, or the node's entry of
 * threshold_map.  The state starts as onset = NONE (0xFFFFFFFF), peak = +0.0f, peak_capture = NONE, pre = M = E[k] = +0.0, and per
 * capture, in capture order:
 *     a  = fabsf(p_c)
 *     if (a > peak)                    { peak = a; peak_capture = c; }     strict: the FIRST occurrence; a NaN changes nothing
 *     if (onset == NONE && a >= thr)   onset = c;                          the onset capture itself falls into bin 0
 *     sq = (double)p_c * (double)p_c                                       exact
 *     if (onset == NONE)  pre = pre + sq;
 *     else { rel = c - onset;  k = the largest k with edges[k] <= rel;
 *            E[k] = E[k] + sq;  M = M + (double)rel * sq; }                the product is rounded, then the sum; nothing is contracted
 * edges[0] = 0 < edges[1] < ... < edges[n_bins - 1] are in captures behind the onset; the last bin is open-ended.  A loop over the
 * snapshots that evaluates these lines (wayverb_amd/arrival.py: arrival_fold; the float lines on float32 arrays, the rest on float64)
 * reproduces all six outputs BIT FOR BIT.  A threshold of 0 is legal: every onset is then capture 0, `pre` stays +0.0 and with
 * edges[k] = k W the bins are, bit for bit, a decay plan's of the same box, cadence and bin_captures = W.
 *
 *   - 1 <= n_bins <= 16, edges as above, the threshold (and every entry of the map) >= 0 and finite, strides and period >= 1;
 *     otherwise, and for a box that leaves the mesh: WV_E_INVALID_ARGUMENT
 *   - everything (the stage of 16 captures, 64 bytes per node; the state, 28 + 8 n_bins bytes per node; the map's copy, 4 bytes per
 *     node where one is given) is allocated when the plan is set: with no room the call answers WV_E_HIP and leaves the engine and
 *     any earlier plan untouched.  The map is copied: the caller's array is free when the call returns.  A new plan replaces the old
 *     one and forgets its state; a NULL plan stops, forgets and frees (as does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE, and wv_run_group refuses an engine with a plan
 *   - an arrival plan excludes the snapshot plan, the spectrum plan, both kinds of decay plan, the intensity plan and the lateral
 *     plan: every setter answers WV_E_STATE while another plan is active, and wv_last_error names the plan to stop
 *   - after a run that stopped on a flag at step f the state has seen exactly the captures of steps <= f: no onset, peak or sum of a
 *     step that was never committed
 *   - wv_step / wv_swap capture nothing; the plan steps they pass are gaps in the series, and `rel` counts captures, not steps
 *   - captures are numbered with 32 bits: wv_run answers WV_E_STATE rather than take capture 2^32 - 1
 *   - wv_checkpoint folds what is staged and copies all per-node state, the capture count and the next plan step aside (the copy is
 *     allocated by the first checkpoint taken under a plan: WV_E_HIP, engine untouched, when there is no room); wv_rollback puts
 *     them back, and the re-run is bitwise the same.  A plan set AFTER the checkpoint makes wv_rollback answer WV_E_STATE
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * wv_arrival_count: as wv_decay_count.  wv_fetch_arrival: onset, peak, peak_capture, pre and moment are [nz][ny][nx], bins is
 * float64 [n_bins][nz][ny][nx]; ANY destination may be NULL and is then skipped; *captures (may be NULL) = how many captures they
 * hold.  It may be called any time outside wv_run, folds what is staged and leaves the plan running.  The step of a node's onset is
 * first_step + onset * period when the run was one wv_run after another from the step the plan was set at. */
typedef struct wv_arrival_plan {
    int32_t x0, y0, z0;    /* first node of the box */
    int32_t nx, ny, nz;    /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;    /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;   /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;       /* >= 1 */
    uint32_t n_bins;       /* 1 .. 16 */
    float threshold;       /* >= 0, finite; used where threshold_map is NULL */
    uint32_t edges[16];    /* first relative capture of bin k; edges[0] == 0, strictly increasing over n_bins entries */
} wv_arrival_plan;
int wv_set_arrival(wv_engine* e, const wv_arrival_plan* plan, const float* threshold_map /* [nz][ny][nx] or NULL; every entry >= 0, finite */);
int wv_arrival_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_arrival(wv_engine* e, uint32_t* onset, float* peak, uint32_t* peak_capture, double* pre, double* moment,
                     double* bins /* [n_bins][nz][ny][nx] */, uint64_t* captures);

/* ---- lateral maps: velocity moments binned from each node's own onset -------------------------- */
/* The early lateral energy fraction LF (J_LF, ISO 3382-1) is the energy a figure-of-eight microphone hears between 5 and 80 ms
 * behind the direct sound over what an omnidirectional one hears in 0 .. 80 ms, AT THAT SEAT.  A figure-of-eight's signal is a
 * component of the particle velocity, so its energy is quadratic in v: an intensity plan, which keeps p v, cannot give it, and bins
 * by one global clock; an arrival plan has each node's own clock and sees pressure only.  A lateral plan has the engine capture a
 * box exactly as an intensity plan captures it, run the reference's directional_receiver integrator at every node taken and keep,
 * per node and on the device, in bins counted from the node's OWN onset: the squared pressure E, the intensity I = p v, and the
 * symmetric second-moment tensor Q = v v^T.  With the tensor the lateral axis d is chosen AFTER the run and per seat (d^T Q d is
 * the figure-of-eight's energy along d, up to (rho c)^2), facing wherever the first bin's intensity says the direct sound came
 * from; its trace is the kinetic half of the energy density.  36 + 80 n_bins bytes per node cross the link when the caller asks,
 * however long the run; wayverb_amd/lateral.py turns them into LF, the direct direction and the diffuseness.
 *
 * wv_lateral_plan holds wv_intensity_plan's box, strides, first_step, period, spacing, sample_rate and ambient_density with the same
 * meaning, and wv_arrival_plan's n_bins, threshold and edges with the same meaning (8 bins at the most).
 *
 * Definition.  pressure, gx, gy, gz are the four floats of the intensity block's first three lines above for the node (the same
 * casts, the same association); c = 0, 1, ... counts the committed captures since the plan was set.  thr is the node's threshold:
 * the plan's scalar, or the node's entry of threshold_map, as wv_set_arrival has it.  The state starts as onset = NONE (0xFFFFFFFF),
 * pre = v[i] = +0.0 and every bin +0.0, and per capture, in capture order:
 *     a = fabsf(pressure)
 *     if (onset == NONE && a >= thr)  onset = c;                  the onset capture itself falls into bin 0; a NaN is no onset
 *     m = (double)g[i] * 0.5;  v[i] = v[i] - m / k;               i = x, y, z; k = ambient_density * sample_rate, an IEEE division;
 *                                                                 EVERY capture, before the onset too
 *     p = (double)pressure
 *     if (onset == NONE)  pre = pre + p * p;
 *     else { rel = c - onset;  b = the largest b with edges[b] <= rel;
 *            E[b]   = E[b]   + p * p;
 *            Ii[b]  = Ii[b]  + v[i] * p;                          the product is rounded, then the sum
 *            Qij[b] = Qij[b] + v[i] * v[j]; }                     (i, j) = xx, yy, zz, xy, xz, yz, in that order
 * edges[0] = 0 < edges[1] < ... < edges[n_bins - 1] are in captures behind the onset; the last bin is open-ended.  Nothing is
 * contracted.  A NumPy loop over snapshots of the box's hull that evaluates these lines (wayverb_amd/lateral.py: lateral_fold; the
 * float lines on float32 arrays, the rest on float64) reproduces onset, pre, v and all ten bin planes BIT FOR BIT.  A threshold of 0
 * is legal: every onset is then capture 0, and with edges[b] = b W the planes E and I and the velocities are, bit for bit, an
 * intensity plan's of the same box, cadence and bin_captures = W; with any threshold onset, pre and E are an arrival plan's.
 *
 *   - 1 <= n_bins <= 8, edges as above, the threshold (and every entry of the map) >= 0 and finite, strides and period >= 1, and
 *     spacing, sample_rate, ambient_density positive and finite; otherwise, and for a box that leaves the mesh: WV_E_INVALID_ARGUMENT
 *   - a taken node with a neighbour off the grid answers WV_E_INVALID_ARGUMENT with the reference's sentence ("Can't place
 *     directional_receiver at this node as it is adjacent to a boundary."), as wv_set_intensity does: no taken node lies on a face of
 *     the mesh.  Neighbours inside a wall are read as the field holds them
 *   - everything (the stage of 16 captures, 256 bytes per node; the state, 36 + 80 n_bins bytes per node; the map's copy, 4 bytes
 *     per node where one is given) is allocated when the plan is set: with no room the call answers WV_E_HIP and leaves the engine
 *     and any earlier plan untouched.  The map is copied: the caller's array is free when the call returns.  A new plan replaces the
 *     old one and forgets its state; a NULL plan stops, forgets and frees (as does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE, and wv_run_group refuses an engine with a plan
 *   - a lateral plan excludes the snapshot plan, the spectrum plan, both kinds of decay plan, the intensity plan and the arrival
 *     plan: every setter answers WV_E_STATE while another plan is active, and wv_last_error names the plan to stop
 *   - after a run that stopped on a flag at step f the state has seen exactly the captures of steps <= f: no onset, velocity or sum
 *     of a step that was never committed
 *   - wv_step / wv_swap capture nothing; the plan steps they pass are gaps in the series, and `rel` counts captures, not steps
 *   - captures are numbered with 32 bits: wv_run answers WV_E_STATE rather than take capture 2^32 - 1
 *   - wv_checkpoint folds what is staged and copies all per-node state, the capture count and the next plan step aside (the copy is
 *     allocated by the first checkpoint taken under a plan: WV_E_HIP, engine untouched, when there is no room); wv_rollback puts
 *     them back, and the re-run is bitwise the same.  A plan set AFTER the checkpoint makes wv_rollback answer WV_E_STATE
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * What the caller owns: the integrator sees a series sampled at sample_rate / period, as under an intensity plan: pass THAT rate.
 *
 * wv_lateral_count: as wv_decay_count.  wv_fetch_lateral: onset and pre are [nz][ny][nx], velocity is float64 [3][nz][ny][nx], bins is
 * float64 [10][n_bins][nz][ny][nx] = E, Ix, Iy, Iz, Qxx, Qyy, Qzz, Qxy, Qxz, Qyz; ANY destination may be NULL and is then skipped;
 * *captures (may be NULL) = how many captures they hold.  It may be called any time outside wv_run, folds what is staged and leaves
 * the plan running. */
typedef struct wv_lateral_plan {
    int32_t x0, y0, z0;    /* first node of the box */
    int32_t nx, ny, nz;    /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;    /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;   /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;       /* >= 1 */
    uint32_t n_bins;       /* 1 .. 8 */
    float threshold;       /* >= 0, finite; used where threshold_map is NULL */
    uint32_t edges[8];     /* first relative capture of bin b; edges[0] == 0, strictly increasing over n_bins entries */
    double spacing;        /* mesh_descriptor::spacing, > 0 */
    double sample_rate;    /* of the CAPTURED series: the mesh's sample rate / period, > 0 */
    double ambient_density;/* > 0 */
} wv_lateral_plan;
int wv_set_lateral(wv_engine* e, const wv_lateral_plan* plan, const float* threshold_map /* [nz][ny][nx] or NULL; every entry >= 0, finite */);
int wv_lateral_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_lateral(wv_engine* e, uint32_t* onset, double* pre, double* velocity /* [3][nz][ny][nx] */,
                     double* bins /* [10][n_bins][nz][ny][nx] */, uint64_t* captures);

/* ---- modulation maps: per-band modulation transfer function of a box, on the device ------------- */
/* How well speech is understood at a seat is the speech transmission index (STI, IEC 60268-16).  Its indirect method derives STI from
 * an impulse response through Schroeder's modulation transfer function, per octave band k and modulation frequency F:
 *     m_k(F) = | sum_t h_k(t)^2 e^(-2 pi i F t) | / sum_t h_k(t)^2
 * with h_k the response filtered into band k.  A decay plan's bins lose the phase this needs, a spectrum plan transforms p and not the
 * band-filtered p^2, and snapshots at period 1 cross the link at 4 bytes per node and step.  A modulation plan has the engine capture
 * the box as a snapshot plan would and keep, per node taken and per band, ON THE DEVICE: the energy and the running Fourier sums of the
 * band-filtered, squared captures at n_freqs modulation frequencies.  8 n_bands (1 + 2 n_freqs) bytes per node cross the link when the
 * caller fetches them, however long the run.  wayverb_amd/modulation.py turns them into the MTF and the STI.
 *
 * Definition.  p_j is the snapshot float of committed capture j (the snapshot block above), n_j its plan step, and x = (double)p_j.
 * For band k the sections s = 0 .. n_sections - 1 run in series on the node's own state z1[k][s], z2[k][s], which starts at +0.0;
 * every product and sum is rounded on its own, nothing is contracted, in wv_set_decay_bands' association:
 *     out = x * b0 + z1
 *     z1  = (x * b1 - a1 * out) + z2
 *     z2  = x * b2 - a2 * out
 *     x   = out                                                     (into the next section)
 * and with y = x after the last section, in capture order, the sums starting at +0.0:
 *     e        = y * y                                              (rounded)
 *     E[k]     = E[k] + e
 *     (c, s)   = wv_spectrum_twiddle(f_m, n_j)                      m = 0 .. n_freqs - 1, f_m in cycles per STEP, 0 <= f_m <= 0.5
 *     Re[k][m] = Re[k][m] + e * c                                   (the product is rounded, then the sum)
 *     Im[k][m] = Im[k][m] - e * s
 * The twiddles are the spectrum plan's, made on the host by the same exported function: the device evaluates no trigonometric
 * function.  A loop over the snapshots of the same plan that evaluates these lines on float64 arrays with the twiddles of
 * wv_spectrum_twiddle (wayverb_amd/modulation.py: modulation_fold) reproduces E, Re and Im BIT FOR BIT; the filter states are
 * reproduced with them, implicitly: mid-run fetches and checkpoints carry them.
 *
 *   - 1 <= n_bands <= 8, 1 <= n_sections <= 4, 1 <= n_freqs <= 16, every coefficient finite; otherwise, and for a NaN or a frequency
 *     outside [0, 0.5], a box that leaves the mesh, a zero stride or a zero period: WV_E_INVALID_ARGUMENT
 *   - everything is allocated when the plan is set: the stage (64 bytes per node), 8 n_bands (1 + 2 n_freqs) bytes of sums and
 *     16 n_sections n_bands bytes of filter state per node, the coefficient table and the two twiddle tables.  With no room the call
 *     answers WV_E_HIP and leaves the engine and any earlier plan untouched.  A new plan replaces the old one and forgets its sums; a
 *     NULL plan stops, forgets and frees (as does wv_destroy)
 *   - box, stride and cadence are the decay plan's; one domain only: a slab of a chain answers WV_E_STATE, and wv_run_group refuses
 *     an engine with a plan
 *   - a modulation plan excludes every other plan -- snapshot, spectrum, both kinds of decay plan, intensity, arrival, lateral: every
 *     setter answers WV_E_STATE while another plan is active, and wv_last_error names the plan to stop
 *   - after a run that stopped on a flag at step f (an overflow, or keep_going cleared) sums and filter states hold exactly the
 *     captures of steps <= f: a continued run goes on as if the dropped captures had never been taken
 *   - wv_step / wv_swap capture nothing; the plan steps they pass are gaps in the series
 *   - wv_checkpoint folds what is staged and copies sums AND filter states, the capture count and the next plan step aside (the copy
 *     is allocated by the first checkpoint taken under a plan: WV_E_HIP, engine untouched, when there is no room); wv_rollback puts
 *     them back, and the re-run is bitwise the same.  A plan set AFTER the checkpoint makes wv_rollback answer WV_E_STATE
 *   - wv_fetch_modulation may be called any time outside wv_run; it folds what is staged and leaves the plan running, so fetching
 *     twice during a long run gives two consistent partial sums
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * What the caller owns.  The series the filters see is sampled at sample_rate / period: design the sections for THAT rate.  With
 * period > 1 field content above sample_rate / (2 period) aliases into the bands, so an impulse source needs period = 1, while a
 * source band-limited below sample_rate / 6 can run at period = 3 and keep three-step passes.  The modulation frequencies are in
 * cycles per STEP whatever the period: F hertz is F / sample_rate.  Auditory masking, the reception threshold and noise need absolute
 * levels and are not part of this: it is the level-independent indirect method.
 *
 * wv_modulation_count: as wv_decay_count.  wv_fetch_modulation: energy is float64 [n_bands][nz][ny][nx], sums is complex128
 * [n_bands][n_freqs][nz][ny][nx] (re, im interleaved); EITHER destination may be NULL and is then skipped; *captures (may be NULL) =
 * how many captures they hold. */
typedef struct wv_modulation_plan {
    int32_t x0, y0, z0;    /* first node of the box */
    int32_t nx, ny, nz;    /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;    /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;   /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;       /* >= 1 */
    uint32_t n_freqs;      /* M, 1 .. 16 */
    uint32_t reserved;
} wv_modulation_plan;
int wv_set_modulation(wv_engine* e, const wv_modulation_plan* plan, const double* cycles_per_step /* [n_freqs] */,
                      const wv_biquad* sections /* [n_bands][n_sections] */, uint32_t n_bands, uint32_t n_sections);
int wv_modulation_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_modulation(wv_engine* e, double* energy /* [n_bands][nz][ny][nx] */,
                        double* sums /* [n_bands][n_freqs][nz][ny][nx][2]: complex128 */, uint64_t* captures);

/* ---- band-limited arrival maps: octave-band clarity, centre time and decay per seat, from one run -- */
/* ISO 3382-1 quotes its figures per octave band.  A banded decay plan gives EDT / T20 / T30 per band; an arrival plan gives C50 / C80,
 * D50 and Ts broadband only, with the dispersive top of an impulse-driven mesh's spectrum in both windows; and the plans exclude each
 * other, so both families cost two runs.  wv_set_arrival_bands is the arrival plan with the banded decay plan's filter bank ahead of
 * the square, and a bin table that can carry a uniform tail behind the explicit edges: per node the BROADBAND onset and peak, and
 * per band the energy ahead of the onset, the first time moment and the squares binned from the node's own onset -- the early windows
 * and the Schroeder curve behind them.  8 + 4 + 8 n_bands (2 + n_bins) bytes per node cross the link when the caller asks.
 *
 * Definition.  p_c is the float a snapshot of the same plan holds for the node; c = 0, 1, ... counts the committed captures since the
 * plan was set; thr as in the arrival plan.  n_bins = n_edges + n_tail.  The state starts as onset = NONE (0xFFFFFFFF), peak = +0.0f,
 * peak_capture = NONE, every pre[k] = M[k] = E[k][b] = z1 = z2 = +0.0, and per capture, in capture order:
 *     a = fabsf(p_c);  if (a > peak) { peak = a; peak_capture = c; }      strict: the FIRST occurrence; a NaN changes nothing
 *     if (onset == NONE && a >= thr) onset = c;                           the BROADBAND onset, one per node, as wv_set_arrival finds it
 *     for every band k:
 *         x = (double)p_c;  n_sections sections in series, exactly wv_set_decay_bands' three lines per section, nothing contracted;
 *         y = x after the last;  sq = y * y                               (rounded)
 *         if (onset == NONE)  pre[k] = pre[k] + sq;
 *         else { d = c - onset;  rel = d > lag[k] ? d - lag[k] : 0;
 *                b = bin(rel);  E[k][b] = E[k][b] + sq;  M[k] = M[k] + (double)rel * sq; }
 *     bin(rel) = (n_tail > 0 && rel >= tail_first) ? n_edges + min((rel - tail_first) / tail_captures, n_tail - 1)
 *                                                  : the largest j with edges[j] <= rel
 * The filters run from capture 0 on every node, before and after its onset.  Windows are counted from the broadband onset, as ISO
 * practice has it; a causal band filter delivers the direct sound late, so the captures [onset, onset + lag[k]) stay in bin 0 with
 * rel = 0 -- no early energy is lost to `pre`, and the window's far edge moves by the lag.  lag = 0 is the plain reading.  A NumPy loop
 * that evaluates these lines (wayverb_amd/arrival.py: banded_arrival_fold; the onset and peak lines on float32, the rest on float64)
 * reproduces every output AND the filter states BIT FOR BIT.  Two consequences, both bytewise:
 *   1. identity sections reproduce the arrival plan: with one band, lag = 0, n_tail = 0 and the section b0 = 1, b1 = b2 = a1 = a2 = 0,
 *      y == x and all six outputs equal wv_set_arrival's with the same edges and threshold
 *   2. threshold 0 reproduces the banded decay plan: with threshold 0, n_edges = 1, tail_first = tail_captures = W and n_tail = n - 1
 *      every onset is capture 0 and the bins equal wv_set_decay_bands' with bin_captures = W, n_bins = n
 *
 * Refused with WV_E_INVALID_ARGUMENT, in this order: a zero stride, a zero period, a box that leaves the mesh (the shared checks);
 * n_bands outside 1 .. 8, n_sections outside 1 .. 4, a coefficient that is not finite; n_edges outside 1 .. 16, edges[0] != 0 or
 * edges not strictly increasing, a threshold (or an entry of the map) that is negative or not finite; n_tail > 4096 - n_edges, with
 * a tail tail_first <= edges[n_edges - 1] or tail_captures == 0, reserved != 0.  Everything else is the arrival plan's rule, word for
 * word: everything is allocated when the plan is set (the stage, 64 bytes per node; 12 + 8 n_bands (2 + n_bins) + 4 n_bands bytes of
 * sums -- every band keeps a copy of the onset -- and 16 n_sections n_bands bytes of filter state per node; the map's copy), and with
 * no room the call answers WV_E_HIP and leaves the engine and any earlier plan untouched; a NULL plan stops, forgets and frees; one
 * domain only, and wv_run_group refuses an engine with a plan; the plan excludes every other plan and every other setter answers
 * WV_E_STATE while it is active; wv_step / wv_swap capture nothing; captures are numbered with 32 bits; after a stop on a flag at step
 * f nothing of a later step is in any sum OR any filter state; wv_checkpoint folds what is staged and copies sums and filter states
 * aside, wv_rollback puts them back; with a plan the fields, receiver rows and flags are bit-identical to a run without one.
 *
 * wv_arrival_bands_count: as wv_decay_count.  wv_fetch_arrival_bands: onset, peak and peak_capture are [nz][ny][nx], pre and moment
 * float64 [n_bands][nz][ny][nx], bins float64 [n_bands][n_bins][nz][ny][nx]; ANY destination may be NULL and is then skipped.
 * The struct is 176 bytes: nine int32 from 0, first_step at 40, period at 48, n_edges at 56, threshold at 60, edges at 64, n_tail at
 * 128, tail_first at 132, tail_captures at 136, lag at 140, reserved at 172. */
typedef struct wv_arrival_bands_plan {
    int32_t x0, y0, z0;      /* first node of the box */
    int32_t nx, ny, nz;      /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;      /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;     /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;         /* >= 1 */
    uint32_t n_edges;        /* 1 .. 16 explicit bins */
    float    threshold;      /* >= 0, finite; used where threshold_map is NULL */
    uint32_t edges[16];      /* edges[0] == 0, strictly increasing over n_edges entries: captures behind the onset */
    uint32_t n_tail;         /* 0 .. 4096 - n_edges uniform bins behind the explicit ones */
    uint32_t tail_first;     /* n_tail > 0: first relative capture of tail bin 0, > edges[n_edges - 1] */
    uint32_t tail_captures;  /* n_tail > 0: W >= 1 captures per tail bin; the LAST bin of the plan is open-ended */
    uint32_t lag[8];         /* per band: captures by which the band's clock starts late (the filter's delay); entries >= n_bands ignored */
    uint32_t reserved;       /* 0 */
} wv_arrival_bands_plan;
int wv_set_arrival_bands(wv_engine* e, const wv_arrival_bands_plan* plan, const float* threshold_map /* [nz][ny][nx] or NULL */,
                         const wv_biquad* sections /* [n_bands][n_sections] */, uint32_t n_bands, uint32_t n_sections);
int wv_arrival_bands_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_arrival_bands(wv_engine* e, uint32_t* onset, float* peak, uint32_t* peak_capture /* [nz][ny][nx] */,
                           double* pre, double* moment /* [n_bands][nz][ny][nx] */,
                           double* bins /* [n_bands][n_bins][nz][ny][nx] */, uint64_t* captures);

/* ---- waterfall maps: time-binned field spectra folded on the device ------------------------------ */
/* How long each MODE of a room rings, and where: below the cutoff the response is a handful of modes, an octave filter is far wider
 * than their spacing, and the whole-run spectrum above has no time axis.  What is drawn for this is a waterfall -- the short-time
 * spectrum, or its cumulative form, the cumulative spectral decay (CSD).  A waterfall plan captures a box of the field exactly as a
 * spectrum plan does (the same nine box ints, the same cadence, the same capture kernel, the same stage of 16 captures) and
 * accumulates, per node taken, per time bin b and per frequency k, a complex Fourier sum ON THE DEVICE.
 *
 * Definition.  p_j is the float a snapshot of plan step n_j holds for the node; j counts the committed captures since the plan was
 * set; b(j) = min(j / bin_captures, n_bins - 1), the decay plan's rule: the last bin is open-ended; (c, s) = wv_spectrum_twiddle(f_k,
 * n_j), with the ABSOLUTE step in the phase.  In capture order, in double, each product rounded, then each sum rounded:
 *     re[b(j)][k] = re[b(j)][k] + (double)p_j * c          im[b(j)][k] = im[b(j)][k] - (double)p_j * s
 * All sums start at +0.0 and a bin no capture reached stays +0.0.  A loop over the snapshots of the same plan that evaluates
 * `a + p * c` on float64 arrays reproduces every sum BIT FOR BIT (wayverb_amd/waterfall.py: waterfall_fold).  It follows that
 *   - n_bins = 1 is the spectrum plan: the bytes are wv_fetch_spectrum's of an identical engine
 *   - Y[b][k] = sum over b' >= b of X[b'][k] is the Fourier transform of the response with everything before capture
 *     b * bin_captures cut away -- the cumulative spectral decay at the bin edges; the absolute phase makes the bins add coherently,
 *     so Y[0] is the whole-run spectrum but for the order of summation
 *   - |X[b][k]|^2 is the short-time spectrum under a rectangular window of bin_captures captures, no overlap.  No window is applied:
 *     the cadence is the caller's tool, as for the spectrum plan.
 *
 *   - 1 <= n_freqs <= 64, 1 <= n_bins <= 4096, bin_captures >= 1, n_freqs * n_bins <= 4096 (64 KiB of sums per node); a frequency
 *     outside [0, 0.5], a NaN, a box that leaves the mesh, a zero stride or a zero period: WV_E_INVALID_ARGUMENT
 *   - everything (the stage of 16 captures, 64 bytes per node; the sums, 16 n_freqs n_bins bytes per node) is allocated when the plan
 *     is set: with no room the call answers WV_E_HIP ("wv_set_waterfall: no room for the stage and the sums") and leaves the engine
 *     and any earlier plan untouched.  A new plan replaces the old one and forgets its sums; a NULL plan stops, forgets and frees (as
 *     does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE (the snapshot plan's reason)
 *   - EXCLUSIVE with every other plan: all decide where passes end; setting one while another is active answers WV_E_STATE
 *   - after a run that stopped on a flag at step f (an overflow, or keep_going cleared) the sums hold exactly the captures of steps
 *     <= f, and wv_waterfall_count says how many: a capture of a step that was never committed is never folded in
 *   - wv_step / wv_swap capture nothing; plan steps they pass are passed, as for snapshots
 *   - wv_checkpoint copies the sums and the count aside (the copy is allocated by the first checkpoint taken under a plan: WV_E_HIP,
 *     engine untouched, when there is no room); wv_rollback puts both back, and the re-run reproduces them bitwise.  A plan set
 *     AFTER the checkpoint makes wv_rollback answer WV_E_STATE, as a changed source does
 *   - wv_fetch_waterfall may be called any time outside wv_run; it folds what is staged and leaves the plan running
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * wv_waterfall_count: as wv_spectrum_count.  wv_fetch_waterfall: the sums as complex128 [n_bins][n_freqs][nz][ny][nx] (re, im
 * interleaved), *captures (may be NULL) = how many captures they hold.  The struct is 72 bytes: nine int32 from 0, first_step at 40,
 * period at 48, n_freqs at 56, n_bins at 60, bin_captures at 64, reserved at 68. */
typedef struct wv_waterfall_plan {
    int32_t x0, y0, z0;     /* first node of the box */
    int32_t nx, ny, nz;     /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;     /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;    /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;        /* >= 1 */
    uint32_t n_freqs;       /* K, 1 .. 64 */
    uint32_t n_bins;        /* 1 .. 4096; n_freqs * n_bins <= 4096 */
    uint32_t bin_captures;  /* W >= 1 captures per bin; the last bin is open-ended */
    uint32_t reserved;      /* 0 */
} wv_waterfall_plan;
int wv_set_waterfall(wv_engine* e, const wv_waterfall_plan* plan, const double* cycles_per_step /* [n_freqs] */);
int wv_waterfall_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_waterfall(wv_engine* e, double* dst /* [n_bins][n_freqs][nz][ny][nx][2]: complex128 */, uint64_t* captures);

/* ---- interaural maps: IACF / IACC at every seat, correlated on the device -------------------------- */
/* ISO 3382-1 Annex B reads spatial impression from the inter-aural cross-correlation function IACF and its maximum IACC (early,
 * late, whole).  It is the one family the plans above cannot give: every one of them is quadratic in ONE node's signal, and the IACF
 * is the normalised cross-correlation of TWO points an ear-distance apart at lags of up to +-1 ms.  An interaural plan captures, for
 * every node taken by a box, the field at two nodes -- the node plus ear_a and the node plus ear_b, offsets in MESH NODES, not box
 * strides -- and accumulates energies and lagged products per time bin counted from the node's own onset, ON THE DEVICE.  The
 * waveguide carries the band below the crossover, where the head is small against the wavelength and the inter-aural difference is
 * a time difference between two points in space: two mesh nodes 0.15 - 0.2 m apart are the head-less ("spaced omni") form of the
 * measurement.  It is not a dummy head.  ear_a == ear_b is legal and gives the per-seat autocorrelation (periodicity, echo and
 * flutter detection).  Ears inside a wall read what the field holds there.
 *
 * Definition.  Per taken node n and committed capture c = 0, 1, ... since the plan was set, in order; L = max_lag; thr = the node's
 * entry of threshold_map, or `threshold`; the state starts as onset = NONE (all bits set), everything else +0.0:
 *
 *     a = (float)field[n + ear_a];  b = (float)field[n + ear_b]             the capture: two floats
 *     mag = fmaxf(fabsf(a), fabsf(b))
 *     if (onset == NONE && mag >= thr) onset = c                            unfiltered; a NaN is no onset
 *     xa = cascade(a), xb = cascade(b)                                      doubles; per section, as wv_set_decay_bands:
 *                                                                              out = x * b0 + z1;  z1 = (x * b1 - a1 * out) + z2;
 *                                                                              z2 = x * b2 - a2 * out;  x = out
 *                                                                           one state per ear, the sections shared;
 *                                                                           n_sections == 0: xa = (double)a, xb = (double)b
 *     if (onset == NONE) { pre[0] = pre[0] + xa * xa;  pre[1] = pre[1] + xb * xb; }
 *     else { w = the largest w with edges[w] <= c - onset;
 *            Ea[w] = Ea[w] + xa * xa;  Eb[w] = Eb[w] + xb * xb;  C[w][L] = C[w][L] + xa * xb;
 *            for l = 1 .. L:  C[w][L + l] = C[w][L + l] + ha[l] * xb;       a earlier, b later by l captures: tau = +l
 *                             C[w][L - l] = C[w][L - l] + hb[l] * xa; }     each product rounded, then the sum
 *     for l = L .. 2: ha[l] = ha[l - 1], hb[l] = hb[l - 1];  ha[1] = xa, hb[1] = xb        EVERY capture, before the onset too
 *
 * A product goes to the bin of the LATER sample: this differs from ISO's "window on the left ear's time" by at most L captures at a
 * bin edge.  wayverb_amd/interaural.py (interaural_fold) evaluates these lines in NumPy, the float lines on float32 and the rest on
 * float64, and reproduces onset, pre and all bins BIT FOR BIT; iacf / iacc / iacc_lag there turn the bins into C / sqrt(Ea Eb).
 *
 *   - n_bins 1 .. 4; edges[0] == 0 and strictly increasing; threshold >= 0 and finite; max_lag 0 .. 16; every ear component in
 *     -8 .. 8; n_sections 0 .. 4 (`sections`: that many wv_biquad, finite; ignored when 0); strides and period >= 1; the box inside
 *     the mesh; every taken node plus either ear inside the mesh ("wv_set_interaural: an ear leaves the mesh"); fewer than 2^31 nodes
 *     per plane; every entry of the map >= 0 and finite: WV_E_INVALID_ARGUMENT, looked at in this order
 *   - everything (the stage of 16 captures, 128 bytes per node; the sums; the lag history and the filter states) is allocated when
 *     the plan is set: with no room the call answers WV_E_HIP ("wv_set_interaural: no room for the stage and the state") and leaves
 *     the engine and any earlier plan untouched.  A new plan replaces the old one and forgets its state; a NULL plan stops, forgets
 *     and frees (as does wv_destroy)
 *   - one domain only: a slab of a chain answers WV_E_STATE (the snapshot plan's reason)
 *   - EXCLUSIVE with every other plan: all decide where passes end; setting one while another is active answers WV_E_STATE
 *   - after a run that stopped on a flag at step f (an overflow, or keep_going cleared) the state holds exactly the captures of steps
 *     <= f, and wv_interaural_count says how many
 *   - wv_step / wv_swap capture nothing; plan steps they pass are passed, as for snapshots
 *   - capture numbers are 32 bits: the capture after number 2^32 - 2 is refused (WV_E_STATE)
 *   - wv_checkpoint copies the state and the count aside (the copy is allocated by the first checkpoint taken under a plan);
 *     wv_rollback puts both back, and the re-run reproduces them bitwise.  A plan set AFTER the checkpoint makes wv_rollback answer
 *     WV_E_STATE, as a changed source does
 *   - wv_fetch_interaural may be called any time outside wv_run; it folds what is staged and leaves the plan running
 *   - with no plan nothing is launched, allocated or waited for; with one the fields, receiver rows and flags are bit-identical to
 *     a run without
 *
 * wv_interaural_count: as wv_spectrum_count.  wv_fetch_interaural: onset uint32 [nz][ny][nx] (0xFFFFFFFF: none yet), pre float64
 * [2][nz][ny][nx], bins float64 [n_bins][2 L + 3][nz][ny][nx] in the order Ea, Eb, C[-L] .. C[+L]; any destination may be NULL;
 * *captures (may be NULL) = how many captures they hold.  The struct is 112 bytes: nine int32 from 0, first_step at 40, period at
 * 48, ear_a at 56, ear_b at 68, max_lag at 80, n_bins at 84, threshold at 88, edges at 92, n_sections at 108. */
typedef struct wv_interaural_plan {
    int32_t x0, y0, z0;     /* first node of the box */
    int32_t nx, ny, nz;     /* nodes TAKEN along each axis (after decimation) */
    int32_t sx, sy, sz;     /* take every s-th node along the axis, >= 1 */
    uint64_t first_step;    /* captures at first_step + j * period, j = 0, 1, ... */
    uint64_t period;        /* >= 1 */
    int32_t ear_a[3];       /* x, y, z offset in mesh nodes from a taken node to its first ear, each -8 .. 8 */
    int32_t ear_b[3];       /* ... to its second ear */
    uint32_t max_lag;       /* L, 0 .. 16: lags -L .. L, counted in captures */
    uint32_t n_bins;        /* 1 .. 4 */
    float threshold;        /* >= 0, finite; used where threshold_map is NULL */
    uint32_t edges[4];      /* first relative capture of bin w; edges[0] == 0, strictly increasing over n_bins entries */
    uint32_t n_sections;    /* 0 .. 4 biquad sections of the ONE band-pass cascade both ears share; 0: no filter */
} wv_interaural_plan;
int wv_set_interaural(wv_engine* e, const wv_interaural_plan* plan, const wv_biquad* sections /* [n_sections], NULL when 0 */,
                      const float* threshold_map /* [nz][ny][nx] or NULL; every entry >= 0, finite */);
int wv_interaural_count(wv_engine* e, uint64_t* captures, uint64_t* last_step);
int wv_fetch_interaural(wv_engine* e, uint32_t* onset, double* pre /* [2][nz][ny][nx] */,
                        double* bins /* [n_bins][2 max_lag + 3][nz][ny][nx] */, uint64_t* captures);

/* ---- timing hooks (bench.py) ------------------------------------------------------------------ */
/* Mean duration in ms of the dominant (pressure update) kernel over the launches since the
 * last call, measured with HIP events on the engine's own stream; 0 launches -> 0. */
int wv_kernel_time_ms(wv_engine* e, double* mean_ms, uint64_t* launches);
int wv_enable_kernel_timing(wv_engine* e, int enable);
/* The same plus the number of time steps the timed launches covered: on meshes big enough to be bound
 * by HBM bytes the engine advances TWO steps per pass over the fields (pair_kernels.hip.h; results are
 * bit-identical to single steps), so a launch of the dominant kernel may stand for two steps. */
int wv_kernel_time_detail(wv_engine* e, double* mean_ms, uint64_t* launches, uint64_t* steps);
/* What the engine is doing, for tests and tools (never needed to use it): *value receives
 *   WV_QUERY_PASSES          two-step passes taken since creation
 *   WV_QUERY_XWALL_ENTRIES   wall nodes that work on compact copies in two-step passes right now (0: none / not in use)
 *   WV_QUERY_FIELDS          pressure fields allocated (2, or 4 once two-step passes have been taken)
 *   WV_QUERY_MARCH_LIVE_PERMILLE   rooms that leave part of the mesh outside: the share of the mesh (in wave-sized
 *                            pieces of rows, per 1000) that the two-step march visits; 1000 when it visits everything
 *   WV_QUERY_SWEEP_LIVE_PERMILLE   the same for the single-step sweep's tiles
 *   WV_QUERY_MARCH_ROUNDS    how many times over the two-step march's workgroups fill the chip's workgroup slots (0 before the
 *                            first pass).  A slab with a neighbour marches in two rounds at least where that costs little, so
 *                            that the exchange of its t+1 faces gets a CU before the march ends
 *   WV_QUERY_HALO_WAIT_NS, WV_QUERY_HALO_WAITS   z-slabs with kernel timing on: total time the compute stream stood waiting for
 *                            ghost planes (the part of the halo exchange the interior work did not hide), over that many timed
 *                            waits (every fourth); both reset by wv_kernel_time
 *   WV_QUERY_HALO_EXCHANGES, WV_QUERY_HALO_BYTES_SENT   exchanges issued and bytes handed to neighbours since creation
 *   WV_QUERY_EARLY_PASSES    two-step passes of a slab that ran both exchanges under the march (wv_tuning::slab_early)
 *   WV_QUERY_TRIPLE_PASSES   three-step passes taken since creation (wv_tuning::triple)
 *   WV_QUERY_SNAPSHOT_NS, WV_QUERY_SNAPSHOT_BYTES, WV_QUERY_SNAPSHOTS_TAKEN   since wv_set_snapshots: total time of the capture kernels
 *                            that ran with kernel timing on, bytes captured, snapshots taken
 *   WV_QUERY_WIDE_GATHERS    steps whose receivers (more than 64 columns) were gathered by a launch of their own, one lane per
 *                            column, since creation (receiver_kernels.hip.h); 0 for ever with 64 columns or fewer
 *   WV_QUERY_DIRECTIONAL_LAUNCHES   launches of the directional receivers' integrator since creation (one per batch of wv_run)
 *   WV_QUERY_SPECTRUM_CAPTURES, WV_QUERY_SPECTRUM_FOLDS, WV_QUERY_SPECTRUM_NS   since wv_set_spectrum: captures of completed steps,
 *                            launches of the fold kernel (one per 16 captures at the most, plus those a fetch or a checkpoint asked
 *                            for), total time of the fold kernels that ran with kernel timing on.  (The capture kernel's time under
 *                            a spectrum plan is in neither this nor WV_QUERY_SNAPSHOT_NS: it is the snapshot plan's capture, whose
 *                            time DESIGN.md 4.7 has)
 *   WV_QUERY_DECAY_CAPTURES, WV_QUERY_DECAY_FOLDS, WV_QUERY_DECAY_NS   the same three since wv_set_decay: captures of completed steps,
 *                            launches of the decay plan's fold kernel, their total time with kernel timing on
 *   WV_QUERY_INTENSITY_CAPTURES, WV_QUERY_INTENSITY_FOLDS, WV_QUERY_INTENSITY_NS   the same three since wv_set_intensity
 *   WV_QUERY_INTENSITY_GATHER_NS, WV_QUERY_INTENSITY_GATHERS   total time of the intensity plan's capture kernels that ran with kernel
 *                            timing on, and how many of them that is
 *   WV_QUERY_ARRIVAL_CAPTURES, WV_QUERY_ARRIVAL_FOLDS, WV_QUERY_ARRIVAL_NS   the decay plan's three since wv_set_arrival
 *   WV_QUERY_LATERAL_CAPTURES, WV_QUERY_LATERAL_FOLDS, WV_QUERY_LATERAL_NS, WV_QUERY_LATERAL_GATHER_NS, WV_QUERY_LATERAL_GATHERS
 *                            the intensity plan's five since wv_set_lateral
 *   WV_QUERY_MODULATION_CAPTURES, WV_QUERY_MODULATION_FOLDS, WV_QUERY_MODULATION_NS   the decay plan's three since wv_set_modulation
 *   WV_QUERY_ARRIVAL_BANDS_CAPTURES, WV_QUERY_ARRIVAL_BANDS_FOLDS, WV_QUERY_ARRIVAL_BANDS_NS   the decay plan's three since wv_set_arrival_bands
 *   WV_QUERY_WATERFALL_CAPTURES, WV_QUERY_WATERFALL_FOLDS, WV_QUERY_WATERFALL_NS   the decay plan's three since wv_set_waterfall
 *   WV_QUERY_INTERAURAL_CAPTURES, WV_QUERY_INTERAURAL_FOLDS, WV_QUERY_INTERAURAL_NS   the decay plan's three since wv_set_interaural */
enum { WV_QUERY_PASSES = 0, WV_QUERY_XWALL_ENTRIES = 1, WV_QUERY_FIELDS = 2, WV_QUERY_MARCH_LIVE_PERMILLE = 3,
       WV_QUERY_SWEEP_LIVE_PERMILLE = 4, WV_QUERY_MARCH_ROUNDS = 5, WV_QUERY_HALO_WAIT_NS = 6, WV_QUERY_HALO_WAITS = 7,
       WV_QUERY_HALO_EXCHANGES = 8, WV_QUERY_HALO_BYTES_SENT = 9, WV_QUERY_EARLY_PASSES = 10,
       /* kernel timing on: total time of the two boundary launches of every eighth two-step pass whose march was timed (nodes to t+1 /
        * to t+2), over that many passes; reset by wv_kernel_time */
       WV_QUERY_BOUNDARY1_NS = 11, WV_QUERY_BOUNDARY2_NS = 12, WV_QUERY_BOUNDARY_TIMED = 13,
       WV_QUERY_WHOLE_STEPS = 14 /* single steps taken as one launch each (wv_tuning::whole_step) */,
       WV_QUERY_TRIPLE_PASSES = 15,
       /* kernel timing of the three-step passes (wv_enable_kernel_timing; reset by wv_kernel_time_ms like the rest): total time and count
        * of the timed three-step marches (kept apart from wv_kernel_time_ms's account, which is the two-step march's or the sweep's); of
        * the passes whose parts were timed (every eighth timed pass): their third boundary launch and their third-level fix-up list
        * (WV_QUERY_BOUNDARY1_NS / 2_NS count the first two boundary launches of either kind of pass) */
       WV_QUERY_TRIPLE_MARCH_NS = 16, WV_QUERY_TRIPLE_MARCH_TIMED = 17, WV_QUERY_BOUNDARY3_NS = 18, WV_QUERY_FIXUP3_NS = 19,
       WV_QUERY_TRIPLE_PARTS_TIMED = 20,
       WV_QUERY_SNAPSHOT_NS = 21, WV_QUERY_SNAPSHOT_BYTES = 22, WV_QUERY_SNAPSHOTS_TAKEN = 23,
       WV_QUERY_WIDE_GATHERS = 24, WV_QUERY_DIRECTIONAL_LAUNCHES = 25,
       WV_QUERY_SPECTRUM_CAPTURES = 26, WV_QUERY_SPECTRUM_FOLDS = 27, WV_QUERY_SPECTRUM_NS = 28,
       WV_QUERY_DECAY_CAPTURES = 29, WV_QUERY_DECAY_FOLDS = 30, WV_QUERY_DECAY_NS = 31,
       WV_QUERY_INTENSITY_CAPTURES = 32, WV_QUERY_INTENSITY_FOLDS = 33, WV_QUERY_INTENSITY_NS = 34,
       WV_QUERY_INTENSITY_GATHER_NS = 35, WV_QUERY_INTENSITY_GATHERS = 36,
       WV_QUERY_ARRIVAL_CAPTURES = 37, WV_QUERY_ARRIVAL_FOLDS = 38, WV_QUERY_ARRIVAL_NS = 39,
       WV_QUERY_LATERAL_CAPTURES = 40, WV_QUERY_LATERAL_FOLDS = 41, WV_QUERY_LATERAL_NS = 42,
       WV_QUERY_LATERAL_GATHER_NS = 43, WV_QUERY_LATERAL_GATHERS = 44,
       WV_QUERY_MODULATION_CAPTURES = 45, WV_QUERY_MODULATION_FOLDS = 46, WV_QUERY_MODULATION_NS = 47,
       WV_QUERY_ARRIVAL_BANDS_CAPTURES = 48, WV_QUERY_ARRIVAL_BANDS_FOLDS = 49, WV_QUERY_ARRIVAL_BANDS_NS = 50,
       WV_QUERY_WATERFALL_CAPTURES = 51, WV_QUERY_WATERFALL_FOLDS = 52, WV_QUERY_WATERFALL_NS = 53,
       WV_QUERY_INTERAURAL_CAPTURES = 54, WV_QUERY_INTERAURAL_FOLDS = 55, WV_QUERY_INTERAURAL_NS = 56 };
int wv_query(wv_engine* e, int what, uint64_t* value);
/* hipStreamSynchronize on every engine stream. */
int wv_synchronize(wv_engine* e);
/* Tuning hook for the streaming kernel.  variant 2 = plane sweep, 0 = register z-march, 1 = naive.
 * rows_per_wave in {2,4}; a workgroup is waves_x by waves_y waves; `knob` = rows per XCD stripe
 * (variant 2) or workgroups along z (variant 0); 0 = automatic everywhere. */
int wv_set_stream_tuning(wv_engine* e, int variant, int rows_per_wave, int waves_x, int waves_y, int knob);

/* ---- z-slab halo exchange over RCCL (multi-GPU) ---------------------------- */
#define WV_UNIQUE_ID_BYTES 128
/* The shared library the RCCL entry points are resolved in (dlopen of exactly this path) instead of the librccl the
 * process finds by name; NULL / "" = by name again.  Process-wide, before the first communicator call (WV_E_STATE
 * afterwards).  For deployments with RCCL outside the loader's path -- and for the test stand-ins under tests/mock_rccl. */
int wv_comm_use_library(const char* path);
/* rank 0 creates the id; the caller distributes the bytes (e.g. torch.distributed broadcast) */
int wv_comm_unique_id(void* id_bytes /* [WV_UNIQUE_ID_BYTES] */);
/* Joins a communicator: this engine is slab `rank` of `nranks`, neighbours rank-1 / rank+1. */
int wv_comm_init(wv_engine* e, const void* id_bytes, int rank, int nranks);
int wv_comm_destroy(wv_engine* e);
/* On a chain of nranks > 1 every rank calls wv_run with the same n_steps.  Before each batch of steps the ranks
 * agree (one small all-reduce) on its length -- the ranks that hold the source plane know where the signal ends, and
 * the run ends there on every rank with the same *steps_done, as it does on one device (hard_source.h:18-20) -- and
 * on the form of its steps (two-step passes need every rank's consent); at the end of every batch the per-step flag
 * words are OR-ed over the ranks (one small all-reduce), so a NaN / Inf / bad-boundary flag raised
 * on one slab stops all of them at the same step -- the multi-device form of waveguide.h:100-119.
 *
 * The same chain inside ONE process (several engines on one GPU, or one per GPU of a node driven
 * from one thread): engines[r] is slab r, created with ghost_lo = (r > 0), ghost_hi = (r < n - 1);
 * face planes travel by device-to-device copies instead of RCCL, everything else in a step is the
 * same code.  Slabs joined this way are stepped together with wv_run_group (same contract as wv_run:
 * *steps_done and *flag are those of the chain; receivers are fetched per engine as usual). */
int wv_comm_init_local(wv_engine* const* engines, int32_t n);
int wv_run_group(wv_engine* const* engines, int32_t n, uint64_t n_steps, uint64_t* steps_done, int32_t* flag);

/* Measured device triad a[i] = b[i] + s*c[i] over n_doubles doubles per array (2 reads + 1 write, the
 * stencil's byte mix), mean of `iters` launches: the bandwidth yardstick of SURVEY.md 8(d). */
int wv_measure_triad(int32_t device, uint64_t n_doubles, int32_t iters, double* gb_per_s);

/* ---- transparent sources ------------------------------------------------------------------------ */
/* compressed_rectangular_waveguide::run_hard_source / run_soft_source
 * (src/waveguide/compensation_signal/lib/include/compensation_signal/waveguide.h:42-131): a free-field mesh
 * folded onto x >= y >= z >= 0 of dim = (steps + 1) / 2 shells (shell dim held at 0), stepped 2 * dim times
 * on the device.  Per step k: node 0 of the current field is set to input[k] (WV_SOURCE_HARD) or has it added
 * (WV_SOURCE_SOFT), 0 once the input is over; every node is updated; the fields swap; output[k] = node 0.
 * Bit-identical to the reference's float arithmetic.  `device` as wv_options::device (-1 = current).
 * WV_E_INVALID_ARGUMENT when the two fields (4 * tetrahedron(dim + 1) bytes each) do not fit in the device's
 * free memory (and for steps > 65536); WV_E_NO_DEVICE without a GPU (no CPU fallback). */
int wv_compressed_waveguide_run(int32_t device, uint64_t steps, int32_t source_kind, const float* input,
                                uint64_t n_input, float* output /* [2 * ((steps + 1) / 2)] */);
/* waveguide::make_transparent (src/waveguide/src/make_transparent.cpp:10-30), host only: the response under
 * core::right_hanning(taps) (float, as core/sinc.h:59-72 makes it), convolved with the input (accumulated in
 * double), subtracted from the input: out[i] = (i < n ? input[i] : 0) - conv[i].  taps >= 2. */
int wv_make_transparent(const float* input, uint64_t n, const float* response, uint32_t taps,
                        float* out /* [n + taps - 1] */);

/* ---- unit kernel of the boundary IIR step ------------------------------------------------------- */
/* The reference's `filter_test_2` test kernel (src/waveguide/src/cl/filters.cpp:66-75, launched by
 * tests/rectangular_kernel.cpp:170-190): n_filters independent order-6 filters, each fed
 * input[s][f] for s = 0..n_samples-1; output[s][f] = filter output as float; memory[f][6] is
 * read, advanced and written back.  Runs the same device code as the boundary kernel. */
int wv_filter_test_2(const float* input, float* output, double* memory,
                     const wv_coefficients_canonical* coeffs, uint32_t n_filters, uint32_t n_samples);
/* Row length (in elements) of the stored pressure fields returned by wv_device_buffer:
 * nx rounded up to the wave tile (128 doubles / 256 floats); element (x,y,z) is at
 * (z*ny + y)*pitch + x and the pad columns are zero. */
int wv_field_pitch(wv_engine* e, uint64_t* pitch_elements);

/* ---- host helpers ------------------------------------------------------------------------------ */
/* Synthetic box mesh of SURVEY.md 8(d): planes [z_begin, z_begin+z_count) of a global
 * nx*ny*nz_global box; boundary_index numbered per dimensionality in increasing node index
 * over planes [number_from, number_to) (set_boundary_index,
 * src/waveguide/src/boundary_coefficient_finder.cpp:11-19); nodes outside that range get index 0.
 * counts[3] receives the number of 1D/2D/3D boundary nodes numbered. */
int wv_make_box_nodes(int32_t nx, int32_t ny, int32_t nz_global, int32_t z_begin, int32_t z_count,
                      int32_t number_from, int32_t number_to, wv_condensed_node* nodes,
                      uint64_t counts[3]);

/* ---- mesh set-up (first slice) -------------------------------------------- */
/* From per-node inside flags (what `set_node_inside` yields, mesh_setup_program.cpp:110-140) to
 * the `condensed_node` array: the reference's `set_node_boundary_type` kernel
 * (src/waveguide/src/mesh_setup_program.cpp:66-108,142-172) on the GPU, then `set_boundary_index`
 * as compute_boundary_index_data applies it (boundary_coefficient_finder.cpp:11-19,44-54):
 * counts[0] = 1-D boundary OR re-entrant nodes, counts[1] = 2-D, counts[2] = 3-D.
 * inside: uint8[nx*ny*nz], non-zero = inside the model. */
int wv_classify_nodes(int32_t nx, int32_t ny, int32_t nz, const uint8_t* inside, wv_condensed_node* nodes,
                      uint64_t counts[3]);

/* Second slice: the inside flags themselves, for triangle-soup scenes.
 * vertices: float[n][4] (cl_float3); triangles: uint32[m][4] = {surface, v0, v1, v2}
 * (src/core/include/core/cl/triangle.h:9-14).
 *
 * wv_voxelise (host): the flattened voxel -> triangle-list array of `get_flattened`
 * (src/core/src/spatial_division/voxel_collection.cpp:9-37) over a side^3 grid on [aabb_min,
 * aabb_max]; a triangle is listed in every voxel whose box, padded by 0.001, it overlaps
 * (src/core/include/core/spatial_division/voxelised_scene_data.h:28-44).  Two-call protocol:
 * *needed always receives the word count; nothing is written unless capacity >= *needed.
 *
 * wv_nodes_inside (GPU): the reference's `set_node_inside` kernel
 * (src/waveguide/src/mesh_setup_program.cpp:110-140; voxel ray-parity test
 * src/core/src/cl/voxel.cpp:98-225) for every node of the mesh (nx, ny, nz, min_corner, spacing):
 * inside[i] = 1 / 0. */
int wv_voxelise(const float* vertices, uint32_t n_vertices, const uint32_t* triangles, uint32_t n_triangles,
                const float aabb_min[3], const float aabb_max[3], uint32_t side, uint32_t* out, uint64_t capacity,
                uint64_t* needed);
int wv_nodes_inside(int32_t nx, int32_t ny, int32_t nz, const float min_corner[3], float spacing,
                    const uint32_t* voxel_index, uint64_t n_voxel_words, const float aabb_min[3],
                    const float aabb_max[3], uint32_t side, const uint32_t* triangles, uint32_t n_triangles,
                    const float* vertices, uint32_t n_vertices, uint8_t* inside);

/* Third slice: which scene surface each boundary filter takes -- compute_boundary_index_data
 * (src/waveguide/src/boundary_coefficient_finder.cpp:38-131) and its kernels
 * boundary_coefficient_finder_1d/_2d/_3d (src/waveguide/src/boundary_coefficient_program.cpp:
 * 310-338, 356-413, 429-484; nearest triangle by exact point-triangle distance, :16-143,218-235).
 * nodes: in, boundary_type as wv_classify_nodes leaves it (boundary_index is ignored);
 *        out, boundary_index as `run` wants it (1-D numbering without the re-entrant nodes).
 * b1 [counts[0]][1], b2 [counts[1]][2], b3 [counts[2]][3]: surface index per filter, i.e. the
 * wv_mesh::boundary_indices_* arrays.  counts[] is always written; with b1 = b2 = b3 = NULL the call
 * is a size query.  WV_E_INVALID_ARGUMENT when a capacity (in rows) is too small or when the
 * mesh lacks 1-D, 2-D or 3-D boundary nodes ("No boundaries.", boundary_coefficient_finder.cpp:30-33).
 * Entry 0 of the 1-D array is written by its owner only (the reference lets every inside node race
 * for it). */
int wv_boundary_index_data(int32_t nx, int32_t ny, int32_t nz, const float min_corner[3], float spacing,
                           wv_condensed_node* nodes, const uint32_t* triangles, uint32_t n_triangles,
                           const float* vertices, uint32_t n_vertices, uint32_t* b1, uint64_t capacity_1,
                           uint32_t* b2, uint64_t capacity_2, uint32_t* b3, uint64_t capacity_3,
                           uint64_t counts[3]);

/* The same three stages chained on the device (compute_mesh, src/waveguide/src/mesh.cpp:54-141, as
 * one unit): nothing but the scene goes up and nothing comes down unless asked for.
 *   wv_scene_mesh_create         inside flags -> node types -> numbering -> surfaces per filter, all in
 *                                HBM on `device` (-1 = current); counts[] = rows of the 1-D/2-D/3-D
 *                                boundary arrays; "No boundaries." like the reference when one is 0
 *   wv_scene_mesh_fetch          host copies (any pointer may be NULL): nodes [nx*ny*nz], b1 [c0][1],
 *                                b2 [c1][2], b3 [c2][3] -- identical to the three-call path above
 *   wv_scene_mesh_create_engine  wv_create on the device-resident nodes (options->device is
 *                                overridden by the scene mesh's device)
 */
typedef struct wv_scene_mesh wv_scene_mesh;
int wv_scene_mesh_create(int32_t nx, int32_t ny, int32_t nz, const float min_corner[3], float spacing,
                         const uint32_t* voxel_index, uint64_t n_voxel_words, const float aabb_min[3],
                         const float aabb_max[3], uint32_t side, const uint32_t* triangles, uint32_t n_triangles,
                         const float* vertices, uint32_t n_vertices, int32_t device, wv_scene_mesh** out,
                         uint64_t counts[3]);
int wv_scene_mesh_fetch(const wv_scene_mesh* sm, wv_condensed_node* nodes, uint32_t* b1, uint32_t* b2, uint32_t* b3);
int wv_scene_mesh_create_engine(const wv_scene_mesh* sm, const wv_coefficients_canonical* coefficients,
                                uint32_t num_coefficients, const wv_options* options, wv_engine** out);
void wv_scene_mesh_destroy(wv_scene_mesh* sm);

/* ---- boundary filter design, host side --------------------------------- */
/* arbitrary_magnitude_filter<6> (src/waveguide/include/waveguide/arbitrary_magnitude_filter.h:63-95):
 * (frequency 0..1 = DC..Nyquist, amplitude) points in any order -> order-6 IIR b/a whose magnitude
 * approximates them.  Points outside [0, 1] are dropped, (0,0) and (1,0) are added, the envelope is
 * resampled to 256 points by linear interpolation and fitted by the modified Yule-Walker method
 * (the reference calls itpp::yulewalk; see wayverb_amd/csrc/filter_design.cpp for what is restated). */
int wv_arbitrary_magnitude_filter(const double* frequency, const double* amplitude, uint32_t n_points,
                                  double b[7], double a[7]);
/* is_stable (src/waveguide/include/waveguide/stable.h:43-50) on ascending-power denominator
 * coefficients a[0..n-1] */
int wv_is_stable(const double* a, uint32_t n, int32_t* stable);
/* hrtf_data::hrtf_band_centres (src/hrtf/lib/include/hrtf/multiband.h:13-20): centres of the 8
 * simulation bands over 20 Hz..20 kHz, divided by sample_rate */
int wv_band_centres(double sample_rate, double centres[8]);
/* compute_reflectance_filter_coefficients (fitted_boundary.h:79-104): 8 band absorptions ->
 * pressure reflectance sqrt(1 - absorption) at 2*centre/sample_rate -> the filter above; fails with
 * "Unable to generate stable boundary filter." when the denominator is not stable */
int wv_reflectance_filter(const double absorption[8], double sample_rate, wv_coefficients_canonical* out);
/* to_impedance_coefficients (fitted_boundary.h:21-48): b' = a + b, a' = a - b, scaled by 1/a'[0]
 * when that is non-zero: what wv_mesh::coefficients holds for a surface (mesh.cpp:126-138) */
int wv_impedance_coefficients(const wv_coefficients_canonical* reflectance, wv_coefficients_canonical* impedance);

/* ---- receiver traces -> audio, host side --------------------------------- */
/* postprocessor::directional_receiver::output (src/waveguide/include/waveguide/postprocessor/
 * directional_receiver.h:22-25): what `canonical` collects per step */
typedef struct wv_directional_output {
    float intensity[3];
    float pressure;
} wv_directional_output;
/* The integrator of wv_set_directional_receivers on the host, for columns that come from somewhere else (a chain of slabs records
 * columns): p7[n][7] = the centre and its neighbours (nx, px, ny, py, nz, pz) per step, as wv_fetch_receivers delivers them;
 * velocity[3] is read and advanced (zeros before the first call), so a trace may be fed in pieces; out[n] receives the records.
 * directional_receiver.cpp:29-67: float pressure differences, a double velocity. */
int wv_directional_accumulate(const double* p7 /* [n][7] */, uint64_t n, double spacing, double sample_rate, double ambient_density,
                              double velocity[3] /* in, out */, wv_directional_output* out /* [n] */);
/* bandpass_band (src/waveguide/include/waveguide/bandpass_band.h:11-20) */
typedef struct wv_waveguide_band {
    const wv_directional_output* directional;
    uint64_t n;
    double sample_rate;
    double valid_hz_min, valid_hz_max;
} wv_waveguide_band;
enum { WV_ATTENUATOR_NULL = 0,       /* core::attenuator::null: the pressure itself */
       WV_ATTENUATOR_MICROPHONE = 1  /* core::attenuator::microphone (pointing, shape) */
       /* core::attenuator::hrtf: 8 bands per sample, see the wv_*_hrtf entry points below */ };
enum { WV_FILTER_LOPASS = 0, WV_FILTER_HIPASS = 1, WV_FILTER_BANDPASS = 2 };

/* attenuate / make_attenuate_mapper (src/waveguide/include/waveguide/attenuator.h:13-49;
 * microphone: src/core/src/attenuator/microphone.cpp:18-25), float arithmetic as there.
 * Fails with "Acoustic impedance outside expected range." unless 300 <= Z < 500. */
int wv_attenuate(int32_t method, const float pointing[3], float shape, float acoustic_impedance,
                 const wv_directional_output* in, uint64_t n, float* out);
/* adjust_sampling_rate (src/waveguide/src/config.cpp:29-56): (size_t)(out/in * n) samples of
 * band-limited interpolation scaled by in/out.  *n_out always receives the length; nothing is
 * written unless capacity suffices.  (The reference calls libsamplerate; see postprocess.cpp.) */
int wv_adjust_sampling_rate(const float* in, uint64_t n, double in_sample_rate, double out_sample_rate, float* out,
                            uint64_t capacity, uint64_t* n_out);
/* frequency_domain::filter{best_fft_length(n) << 2}.run with compute_lopass / hipass /
 * bandpass_magnitude as the per-bin gain (src/frequency_domain/src/filter.cpp:22-47,
 * envelope.cpp:60-112); edges relative to the sample rate, in place */
int wv_frequency_domain_filter(float* signal, uint64_t n, int32_t kind, double edge_lo, double edge_hi,
                               double width_factor, uint32_t steepness);
/* waveguide::postprocess(bandpass_bands, method, Z, output_sample_rate)
 * (src/waveguide/include/waveguide/postprocess.h:74-126): attenuate, resample, band-pass each
 * band at its valid range, sum, 10 Hz DC block.  Size-query protocol as above. */
int wv_postprocess_waveguide(const wv_waveguide_band* bands, uint32_t n_bands, int32_t method, const float pointing[3],
                             float shape, float acoustic_impedance, double output_sample_rate, float* out,
                             uint64_t capacity, uint64_t* n_out);

/* ---- HRTF receiver capsules (core::attenuator::hrtf, src/core/include/core/attenuator/hrtf.h) ---------
 * The reference looks the 8 band energies of a direction up in a table it generates AT BUILD TIME from
 * measured head-related impulse responses (src/hrtf/cmd/main.cpp writes hrtf_entries.h; neither that file
 * nor the measurements are in the reference tree), so the table is the caller's to supply:
 *   energy[az][el][channel][band], az in [0, az_num): azimuth az * 360 / az_num degrees,
 *   el in [0, el_num): elevation (el + 1) * 180 / (el_num + 1) - 90 degrees (el_num odd), channel 0 = left,
 *   nearest-entry lookup exactly as vector_look_up_table.h:50-110 (azimuth = atan2(x, -z) negated, elevation =
 *   asin(y), in the head's frame: pointing = -z, up = +y; orientation.cpp:21-43). */
typedef struct wv_hrtf_table {
    const double* energy;
    uint32_t az_num, el_num;
} wv_hrtf_table;
/* attenuation(hrtf, incident) (src/core/src/attenuator/hrtf.cpp:121-133) */
int wv_hrtf_attenuation(const wv_hrtf_table* table, const float pointing[3], const float up[3], int32_t channel,
                        const float incident[3], float bands[8]);
/* get_ear_position (hrtf.cpp:135-141); fails with "Hrtf radius outside reasonable range." unless 0 <= radius <= 1 */
int wv_hrtf_ear_position(const float pointing[3], const float up[3], int32_t channel, float radius,
                         const float base_position[3], float ear[3]);
/* attenuate / make_attenuate_mapper with an hrtf method (attenuator.h:13-49): out[n][8] */
int wv_attenuate_hrtf(const wv_hrtf_table* table, const float pointing[3], const float up[3], int32_t channel,
                      float acoustic_impedance, const wv_directional_output* in, uint64_t n, float* out);
/* core::multiband_filter_and_mixdown (src/core/include/core/mixdown.h:17-26; hrtf_data::multiband_filter,
 * src/hrtf/lib/include/hrtf/multiband.h:38-44): bands[n][8] is filtered in place, out[n] = sum of the 8 bands */
int wv_multiband_filter_and_mixdown(float* bands, uint64_t n, double sample_rate, float* out);
/* waveguide::postprocess with an hrtf method (postprocess.h:57-126).  Size-query protocol as above. */
int wv_postprocess_waveguide_hrtf(const wv_waveguide_band* bands, uint32_t n_bands, const wv_hrtf_table* table,
                                  const float pointing[3], const float up[3], int32_t channel, float acoustic_impedance,
                                  double output_sample_rate, float* out, uint64_t capacity, uint64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* WAYVERB_AMD_H */
