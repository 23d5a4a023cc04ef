// engine.hip.h -- `Engine<Real>`: one `waveguide::run` worth of device state and the host logic that steps it
// (src/waveguide/include/waveguide/waveguide.h:36-126 is what it replaces).  Real = float (the reference's cl_float
// fields) or double (BASELINE.json's fp64 engine).
//
// The member functions are defined in:
//   engine_setup.hip.h   wv_create: buffers, class map, boundary entry lists and their processing order, sweep plan,
//                        work lists for rooms that leave much of the mesh outside; release
//   engine_single.hip.h  one time step per pass: sweep + boundary launches, source / receiver launch, the slab form
//                        (faces first, exchange, interior), hipGraph replay for small meshes
//   engine_pair.hip.h    two time steps per pass: eligibility, pair map + fix-up lists, march geometry, parts A / B; the launch
//                        sequences both kinds of pass share (source / receiver launch, boundary launch that carries one, wall copies)
//   engine_triple.hip.h  three time steps per pass: eligibility, triple map + third-level list, march geometry, the pass
//   march_plan.h         (host only, no HIP) MarchPlan and the planners of both marches: windows of a long row, chunks along z, the
//                        work list of a sparse room, plan -> kernel arguments
//   engine_batch.hip.h   wv_step / wv_run: batches of steps, flag words, kernel timing
//   engine_io.hip.h      everything a caller reads or writes: values, fields, planes, filter memories, source,
//                        receivers
//   engine_snapshot.hip.h  field snapshots taken on the device while a run goes on (wv_set_snapshots): plan, ring, capture, copy stream, held log
//   snapshot_plan.h      (host only, no HIP) which steps are snapshot steps, how far a batch may go, box validity, output shape; what every
//                        plan's setter checks: the box of a plan, the four shared refusals, frequencies, coefficients, physical constants
//   engine_staged.hip.h  the life cycle the nine accumulating plans below share: set, capture, commit, fold, checkpoint, rollback, release;
//                        the host-written tables of a fold (bins, twiddles), the threshold map, the fetch of complex sums
//   fold_parts.hip.h     the device pieces more than one fold kernel has and that leave its assembly alone: stage read, integrator step, onset rule
//   engine_spectrum.hip.h  field spectra accumulated on the device while a run goes on (wv_set_spectrum): plan, stage, fold, fetch
//   spectrum_plan.h      (host only, no HIP) free slots of the stage, when a fold is due, which captures survive a stop, sizes
//   capture_stage.h      (host only, no HIP) the bookkeeping of a stage of captures, shared by the nine accumulating plans
//   engine_decay.hip.h   time-binned field energy accumulated on the device while a run goes on (wv_set_decay): plan, stage, fold, fetch
//   decay_plan.h         (host only, no HIP) the bin of a capture, sizes, the fold's traffic model
//   decay_bands_kernels.hip.h   the fold of a band-limited decay plan (wv_set_decay_bands): biquad cascades ahead of the square
//   engine_intensity.hip.h  time-binned sound intensity of a box accumulated on the device (wv_set_intensity): plan, stage, fold, fetch
//   intensity_plan.h     (host only, no HIP) what an intensity plan is refused for, sizes, the fold's traffic model
//   intensity_kernels.hip.h   its capture (pressure and gradient differences of every taken node) and its fold
//   engine_arrival.hip.h  energy of a box binned from each node's OWN arrival, onset and peak per node (wv_set_arrival): plan, stage, fold, fetch
//   arrival_plan.h       (host only, no HIP) edge tables, the bin of a capture behind an onset, sizes and places, the fold's traffic model
//   arrival_kernels.hip.h     its fold: decay_fold_kernel's scheme with a bin that differs from lane to lane
//   engine_lateral.hip.h  p^2, p v and v v^T of a box binned from each node's OWN arrival (wv_set_lateral): plan, stage, fold, fetch
//   lateral_plan.h       (host only, no HIP) what a lateral plan is refused for, sizes and places, the fold's traffic model
//   lateral_kernels.hip.h     its fold: arrival_fold_kernel's onset and bin around intensity_fold_kernel's integrator
//   engine_modulation.hip.h  band energies and their Fourier sums at modulation frequencies of a box (wv_set_modulation): plan, stage, fold, fetch
//   modulation_plan.h    (host only, no HIP) what a modulation plan is refused for, sizes and places, the fold's traffic model
//   modulation_kernels.hip.h  its fold: decay_bands_fold_kernel's cascade ahead of spectrum_fold_kernel's running Fourier sum
//   engine_arrival_bands.hip.h  per octave band, energy of a box binned from each node's OWN arrival, with a uniform tail (wv_set_arrival_bands)
//   arrival_bands_plan.h  (host only, no HIP) the tail, the bin of a capture behind an onset and a lag, sizes and places, the traffic model
//   arrival_bands_kernels.hip.h  its fold: decay_bands_fold_kernel's cascade ahead of arrival_fold_kernel's onset and bins
//   engine_waterfall.hip.h  per time bin, the Fourier sums of a box at K frequencies: short-time spectra and the cumulative spectral decay (wv_set_waterfall)
//   waterfall_plan.h     (host only, no HIP) the cap on sums per node, sizes and places, the fold's traffic model
//   waterfall_kernels.hip.h   its fold: spectrum_fold_kernel's chunked Fourier sum driven by decay_fold_kernel's held bin
//   engine_interaural.hip.h  per node the energies and lagged products of the field at two nodes an ear-distance apart, binned from the node's own arrival: IACF / IACC (wv_set_interaural)
//   interaural_plan.h    (host only, no HIP) what a plan is refused for and in which order, the lag class, sizes and places, the traffic model
//   interaural_kernels.hip.h  its capture (ear_gather_kernel: the third kind beside the snapshot's and the intensity plan's) and its fold
//   engine_directional.hip.h  receiver arrays: directional receivers recorded and integrated on the device (wv_set_directional_receivers)
//   engine_slab.hip.h    z-slab chains: communicators, the in-process group (wv_comm_init_local / wv_run_group)
// There is no CPU path: without a HIP device every entry point fails.
#pragma once
#include "engine_base.h"
#include "march_plan.h"
#include "snapshot_plan.h"
#include "spectrum_plan.h"
#include "decay_plan.h"
#include "intensity_plan.h"
#include "arrival_plan.h"
#include "lateral_plan.h"
#include "modulation_plan.h"
#include "arrival_bands_plan.h"
#include "waterfall_plan.h"
#include "interaural_plan.h"
#include "capture_stage.h"

#include "boundary_kernels.hip.h"
#include "pair_kernels.hip.h"
#include "stream_kernels.hip.h"
#include "plane_kernels.hip.h"
#include "snapshot_kernels.hip.h"
#include "spectrum_kernels.hip.h"
#include "decay_kernels.hip.h"
#include "decay_bands_kernels.hip.h"
#include "intensity_kernels.hip.h"
#include "arrival_kernels.hip.h"
#include "lateral_kernels.hip.h"
#include "modulation_kernels.hip.h"
#include "arrival_bands_kernels.hip.h"
#include "waterfall_kernels.hip.h"
#include "interaural_kernels.hip.h"
#include "receiver_kernels.hip.h"
#include "triple_kernels.hip.h"

namespace wv {

// (engine_directional.hip.h, engine_slab.hip.h)
constexpr const char* kDirectionalOnSlab =
        "directional receivers on the device: not on a slab of a chain (a receiver next to a cut has a neighbour in a ghost plane); "
        "record the 7 columns per receiver with wv_set_receivers and integrate them with wv_directional_accumulate";

template <typename Real>
class Engine final : public wv_engine {
public:
    ~Engine() override { release(); }
    // ---- engine_setup.hip.h
    int init(const wv_mesh& m, const wv_options& opt) override;
    int set_tuning(int variant, int ry, int nwx, int nwy, int zchunks) override;
    int build_plane_order();
    void plan_stream();
    // ---- engine_single.hip.h
    template <int RY, int NWX, int NWY>
    void launch_shape(const wv::StreamArgs<Real>& a, unsigned grid);
    template <int RY>
    void launch_ry(const wv::StreamArgs<Real>& a, unsigned grid);
    // ---- engine_setup.hip.h
    int build_tile_lists(int z0, int z1);
    // ---- engine_single.hip.h
    // (`plan_only`: the launch's arguments and grid are handed back instead of launched -- launch_faces puts them into one launch
    // with the planes' boundary entries)
    struct StreamLaunch {
        wv::StreamArgs<Real> args;
        unsigned grid = 0;
    };
    int launch_stream(Real* prev, const Real* cur, int* flag, int z0, int z1, bool timed, Real* out = nullptr, int zb0 = 0, int zb1 = 0,
                      StreamLaunch* plan_only = nullptr);
    // (`planes`: how many owned planes next to each neighbour -- 1: the face planes, 2: the faces and the planes next to them)
    int launch_faces(Real* prev, const Real* cur, int* flag, Real* out, int planes = 1);
    wv::BoundaryArgs<Real> boundary_args(Real* prev, const Real* cur, int* flag) const;
    struct BoundaryLaunch {
        wv::BoundaryArgs<Real> args;
        unsigned blocks = 0;
        bool lds = false;
    };
    // What a boundary launch covers and does, by name.
    struct BoundaryPlanes {
        enum Which { range, faces, faces_and_next } which = range;  // [z0, z1) | a slab's face planes | ... and the planes next to them
        int z0 = 0, z1 = 0;
        static BoundaryPlanes of(int z0, int z1) { return {range, z0, z1}; }
        static BoundaryPlanes next_to_neighbours(int planes) { return {planes == 2 ? faces_and_next : faces, 0, 0}; }
    };
    struct XwallUse {  // the x-facing walls by position on their compact copies, in a pass's launch over the bulk of the mesh
        int depth = 0, level = 0;  // none, or the steps of the pass (2, 3) and the level (1..depth) of this launch
    };
    struct BoundarySpec {
        BoundaryPlanes planes;
        Real* out = nullptr;                          // passes: the new values go to another field instead of replacing `prev`
        const wv::PrePostArgs<Real>* ride = nullptr;  // source / receiver work that rides in the launch
        bool fix_inner = false;                       // 1-D entries also finish the inside node they face
        XwallUse copies;
        BoundaryLaunch* plan_only = nullptr;          // hand the launch's arguments and grid back instead of launching
    };
    int launch_boundary(Real* prev, const Real* cur, int* flag, const BoundarySpec& spec);
    wv::PrePostArgs<Real> pre_post_args(Real* cur, int slot, bool with_pre_post, uint64_t signal_pos, bool source_live) const;
    int enqueue_step(int slot, bool with_pre_post, uint64_t signal_pos, bool source_live, int fuse_next = 0);
    // one-launch steps (plane_kernels.hip.h, whole_step_kernel): may this engine take them (synchronises once per source / receiver
    // set: not inside a capture), and the launch itself
    bool whole_step_ready();
    bool whole_step_sized() const;  // small enough for the form to beat two-step passes too (the automatic choice)
    int launch_whole_step(Real* prev, const Real* cur, int slot, uint64_t signal_pos, bool source_live, bool serve_next);
    // ---- engine_pair.hip.h
    bool pair_eligible();
    int ensure_pair();
    int build_pair_units();
    static void parallel_sort(std::vector<uint64_t>& v);
    int enqueue_pair_a(int slot, uint64_t signal_pos, bool source_live, bool fuse_mid);
    int launch_fixup(uint32_t first, uint32_t n, const Real* t1, const Real* cur, Real* out2, int* flag2);
    int build_xwall();
    void xwall_args(wv::BoundaryArgs<Real>& b) const;
    int enqueue_pair_b(int slot, uint64_t signal_pos, bool source_live, int fuse_next);
    bool slab_early_now() const;
    int begin_halo_wait_timing();
    int end_halo_wait_timing(int token);
    int begin_part_timing(int part, bool always = false);
    int end_part_timing(int part, int token);
    int enqueue_batch_pair(uint64_t i, int part, int next_kind) override;
    int batch_pair_eligible(int* eligible) override;
    int batch_pair_prepare(int* ready, int* singles_first) override;
    int batch_pair_vetoed() override;
    int batch_triple_prepare(int* ready) override;
    int enqueue_batch_triple(uint64_t i, int part) override;
    uint64_t role_signature() const override {
        return (uint64_t)cur_ | (uint64_t)prv_ << 2 | (uint64_t)spare_[0] << 4 | (uint64_t)spare_[1] << 6 | steps_done << 8;
    }
    // ---- engine_triple.hip.h
    static constexpr int kWideLaneBytes = 16;  // the wider form of the three-step march's lanes (triple_kernels.hip.h)
    int triple_lane_bytes() const;
    bool triple_eligible();
    int ensure_triple();
    int build_triple_units();
    int enqueue_triple(int slot, uint64_t signal_pos, bool source_live, int fuse_next);
    int enqueue_triple_slab(int slot, int part, uint64_t signal_pos, bool source_live);
    int launch_triple_march(int slot, const Real* A, const Real* B, Real* O1, Real* O2, Real* O3);
    int launch_triple_list(int slot, const Real* A, const Real* B, const Real* O1, const Real* O2, Real* O3, bool source_live);
    // ---- engine_batch.hip.h
    bool time_this_launch();
    int drain_timing();
    int step(int32_t* flag) override;
    int swap() override;
    // ---- engine_single.hip.h
    int replay_batch(uint64_t batch, bool source_live, bool can_fuse);
    // ---- engine_batch.hip.h
    uint64_t plan_batch(uint64_t remaining) override;
    int enqueue_batch_step(uint64_t i, uint64_t batch, int next_kind) override;
    int collect_batch(uint64_t batch) override;
    const int* batch_flags() const override { return flags_host_; }
    int commit_batch(uint64_t batch, const int* flags, uint64_t* good_out, int32_t* flag_out) override;
    int run(uint64_t n_steps, uint64_t* done, int32_t* flag_out) override;
    // ---- engine_io.hip.h
    int set_source(int kind, uint64_t node, const double* signal, uint64_t n) override;
    int set_receivers(const uint64_t* nodes, uint32_t n) override;
    int set_columns(const uint64_t* nodes, uint32_t n);  // what wv_set_receivers does to the recorded columns, in either mode
    bool io_nodes_plain();
    bool io_nodes(std::vector<uint64_t>* stored);
    bool io_nodes_unfaced();
    bool io_nodes_clear_of_x_walls();
    int fetch_receivers(uint64_t first, uint64_t n, double* dst) override;
    Real* buffer(int which) { return which == WV_BUF_CURRENT ? field_[cur_] : field_[prv_]; }
    hipError_t class_of(uint64_t x, uint64_t row, uint32_t* cls);
    uint64_t stored_index(uint64_t node) const;
    int read_value(int buffer_id, uint64_t index, double* v) override;
    int write_value(int buffer_id, uint64_t index, double v) override;
    template <typename Other>
    int copy_field(Real* stored, void* host, bool to_device, int z0, int planes);
    int read_field(int buffer_id, void* dst, int elem_size) override { return read_planes(buffer_id, 0, nz_, dst, elem_size); }
    int write_field(int buffer_id, const void* src, int elem_size) override {
        return write_planes(buffer_id, 0, nz_, src, elem_size);
    }
    int read_planes(int buffer_id, int z0, int planes, void* dst, int elem_size) override;
    int write_planes(int buffer_id, int z0, int planes, const void* src, int elem_size) override;
    int boundary_data(int dim, wv_boundary_data* host, bool to_device) override;
    int set_coefficients(const wv_coefficients_canonical* c, uint32_t n) override;
    int device_buffer(int buffer_id, void** p) override;
    int checkpoint(int op) override;
    // ---- engine_directional.hip.h
    int set_directional_receivers(const uint64_t* nodes, uint32_t n, double spacing, double sample_rate, double ambient_density) override;
    int fetch_directional(uint64_t first, uint64_t n, wv_directional_output* dst) override;
    int fetch_directional_velocity(double* dst) override;
    // ---- engine_snapshot.hip.h
    int set_snapshots(const wv_snapshot_plan* plan) override;
    int snapshot_count(uint64_t* taken, uint64_t* first_held) override;
    int fetch_snapshots(uint64_t first, uint64_t n, float* dst, uint64_t* steps) override;
    bool snapshots_active() const override { return snap_.active; }
    // ---- engine_spectrum.hip.h
    int set_spectrum(const wv_spectrum_plan* plan, const double* cycles_per_step) override;
    int spectrum_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(spec_, captures, last_step); }
    int fetch_spectrum(double* dst, uint64_t* captures) override;
    bool spectrum_active() const override { return spec_.active; }
    // ---- engine_decay.hip.h
    int set_decay(const wv_decay_plan* plan) override;
    int decay_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(decay_, captures, last_step); }
    int fetch_decay(double* dst, uint64_t* captures) override;
    int set_decay_bands(const wv_decay_plan* plan, const wv_biquad* sections, uint32_t n_bands, uint32_t n_sections) override;
    int fetch_decay_bands(double* dst, uint64_t* captures) override;
    bool decay_active() const override { return decay_.active; }
    // ---- engine_intensity.hip.h
    int set_intensity(const wv_intensity_plan* plan) override;
    int intensity_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(inten_, captures, last_step); }
    int fetch_intensity(double* dst, uint64_t* captures) override;
    int fetch_intensity_velocity(double* dst) override;
    bool intensity_active() const override { return inten_.active; }
    // ---- engine_arrival.hip.h
    int set_arrival(const wv_arrival_plan* plan, const float* threshold_map) override;
    int arrival_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(arr_, captures, last_step); }
    int fetch_arrival(uint32_t* onset, float* peak, uint32_t* peak_capture, double* pre, double* moment, double* bins, uint64_t* captures) override;
    bool arrival_active() const override { return arr_.active; }
    // ---- engine_lateral.hip.h
    int set_lateral(const wv_lateral_plan* plan, const float* threshold_map) override;
    int lateral_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(lat_, captures, last_step); }
    int fetch_lateral(uint32_t* onset, double* pre, double* velocity, double* bins, uint64_t* captures) override;
    bool lateral_active() const override { return lat_.active; }
    // ---- engine_modulation.hip.h
    int set_modulation(const wv_modulation_plan* plan, const double* cycles_per_step, const wv_biquad* sections, uint32_t n_bands, uint32_t n_sections) override;
    int modulation_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(mod_, captures, last_step); }
    int fetch_modulation(double* energy, double* sums, uint64_t* captures) override;
    bool modulation_active() const override { return mod_.active; }
    // ---- engine_arrival_bands.hip.h
    int set_arrival_bands(const wv_arrival_bands_plan* plan, const float* threshold_map, const wv_biquad* sections, uint32_t n_bands, uint32_t n_sections) override;
    int arrival_bands_count(uint64_t* captures, uint64_t* last_step) override;
    int fetch_arrival_bands(uint32_t* onset, float* peak, uint32_t* peak_capture, double* pre, double* moment, double* bins, uint64_t* captures) override;
    bool arrival_bands_active() const override { return arrb_.active; }
    // ---- engine_waterfall.hip.h
    int set_waterfall(const wv_waterfall_plan* plan, const double* cycles_per_step) override;
    int waterfall_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(wf_, captures, last_step); }
    int fetch_waterfall(double* dst, uint64_t* captures) override;
    bool waterfall_active() const override { return wf_.active; }
    // ---- engine_interaural.hip.h
    int set_interaural(const wv_interaural_plan* plan, const wv_biquad* sections, const float* threshold_map) override;
    int interaural_count(uint64_t* captures, uint64_t* last_step) override { return staged_count(ia_, captures, last_step); }
    int fetch_interaural(uint32_t* onset, double* pre, double* bins, uint64_t* captures) override;
    bool interaural_active() const override { return ia_.active; }
    // ---- engine_batch.hip.h
    int kernel_time(double* mean_ms, uint64_t* launches, uint64_t* steps) override;
    int synchronize() override;
    int query(int what, uint64_t* value) override;
    // ---- engine_slab.hip.h
    int comm_init(const void* id, int rank, int nranks) override;
    int comm_init_local(int rank, int nranks) override;
    int adopt_comm(std::unique_ptr<wv::SlabComm> c);
    wv::SlabComm* comm() override { return comm_.get(); }
    uint64_t field_pitch() const override { return (uint64_t)pitch_; }
    int comm_destroy() override;

private:
    void release();  // engine_setup.hip.h
    // ---- engine_pair.hip.h: launch sequences the passes share
    void launch_pre_post(const wv::PrePostArgs<Real>& pp);
    void launch_pre_post(Real* field, int slot, uint64_t signal_pos, bool source_live, bool clear_flag, int* flag2 = nullptr, bool with_pre_post = true);
    // who does the source / receiver work that goes with a boundary launch: nobody here, the launch's last workgroup, a launch behind it
    enum class IoRide { none, carried, behind };
    int launch_boundary_with_io(int part, Real* prev, const Real* cur, int* flag, const BoundarySpec& spec, const wv::PrePostArgs<Real>& io, IoRide ride);
    void carry_short_list(wv::PrePostArgs<Real>& io, const Real* cur, Real* out2, int* flag2) const;
    void refresh_xwall_copies(Real* prev, const Real* cur, int* flag);
    void rotate_after_pass();
    int march_activity(int strips, int row_waves, int wave_cols, std::vector<uint8_t>* active, std::vector<uint16_t>* wave_bits);
    int upload_units(const wv::MarchPlan& plan, uint32_t** dev, const char* what);
    // rooms that leave much of the mesh outside: visit live tiles / units only (wv_options::all_tiles, wv_tuning::tile_lists)
    bool use_work_lists() const { return !opt_.all_tiles && opt_.tuning.tile_lists != 0; }

    wv_options opt_{};
    int nx_ = 0, ny_ = 0, nz_ = 0, z_begin_ = 0, z_end_ = 0, device_ = -1;
    uint64_t n_nodes_ = 0, stored_nodes_ = 0, field_bytes_ = 0;
    int pitch_ = 0;
    Real* field_[4] = {nullptr, nullptr, nullptr, nullptr};
    int cur_ = 1, prv_ = 0, spare_[2] = {2, 3};  // which field_ holds which role
    uint8_t* cls_ = nullptr;
    int cls_pitch_ = 0;
    uint32_t n1_ = 0, n2_ = 0, n3_ = 0, n_entries_ = 0, n_slots_ = 0, n_coeffs_ = 0;
    uint32_t* bnode_ = nullptr;
    uint64_t* tile_list_ = nullptr;   // sweep work list (build_tile_lists), null = arithmetic mapping
    uint32_t list_start_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t list_longest_ = 0;
    bool lists_built_ = false;
    int lists_z0_ = 0, lists_z1_ = 0;  // plane range the lists were built for
    struct GraphKey {
        uint64_t batch;
        int cur;
        bool source_live, can_fuse;
        uint32_t n_recv;
        uint64_t source_node;
        int source_kind;
        uint64_t signal_ptr, recv_ptr;
        bool lists;
        uint64_t cur_ptr, prv_ptr;
        uint64_t io_generation;  // set_source / set_receivers calls so far: the one-launch steps' duty count and legality are baked into the capture
        bool operator==(const GraphKey& o) const {
            return batch == o.batch && cur == o.cur && source_live == o.source_live && can_fuse == o.can_fuse &&
                   n_recv == o.n_recv && source_node == o.source_node && source_kind == o.source_kind &&
                   signal_ptr == o.signal_ptr && recv_ptr == o.recv_ptr && lists == o.lists && cur_ptr == o.cur_ptr &&
                   prv_ptr == o.prv_ptr && io_generation == o.io_generation;
        }
    };
    hipGraphExec_t graph_exec_ = nullptr;
    GraphKey graph_key_{};
    uint64_t* signal_base_dev_ = nullptr;
    bool graph_capturing_ = false;
    uint64_t graph_max_nodes_ = 64ull << 20;
    bool batch_flags_reset_ = false;  // the flag words of the batch being enqueued hold the mesh-static bits already
    bool pre_post_done_ = false;      // this step's pre/post work was done by the previous boundary launch
    // two-step passes
    int pair_inner_ok_ = -1;  // boundary entries finish the inside nodes they face (ensure_pair): -1 not checked yet
    uint64_t pair_min_nodes_ = 4ull << 20;      // stored nodes: between 128^3 (single steps win) and 160^3 (passes win)
    bool pair_failed_ = false;
    uint8_t* pair_map_ = nullptr;
    uint32_t* pair_list_ = nullptr;
    uint32_t* pair_counter_ = nullptr;
    wv::MarchPlan pair_plan_;                      // the two-step march: planes, geometry, windows, work list (ensure_pair, build_pair_units)
    uint32_t* pair_units_ = nullptr;               // its work list on the device, null = every unit
    bool pair_sparse_ok_ = true;                   // sparse room: the march's live units cost less than the sweep's live tiles
    double tile_active_frac_ = 1.0;
    uint32_t pair_list_n_ = 0;  // fix-up nodes of the marched planes
    uint64_t pair_source_ = 0;
    uint64_t timed_steps_ = 0;
    bool batch_can_fuse_ = false, batch_source_live_ = false;  // plan_batch's decisions for the batch being enqueued
    bool io_plain_known_ = false, io_plain_ = false;
    bool io_unfaced_known_ = false, io_unfaced_ = false;
    bool io_xclear_known_ = false, io_xclear_ = false;  // io_nodes_clear_of_x_walls
    bool duties_known_ = false, duties_ok_ = false;  // whole_step_ready
    wv::StepDuty* duties_ = nullptr;                  // [n_duties_] the source first, then the recorded receivers
    uint32_t n_duties_ = 0;
    uint64_t whole_steps_ = 0;                        // steps taken as one launch (WV_QUERY_WHOLE_STEPS)
    uint64_t graph_whole_steps_ = 0;                  // ... by one replay of the captured batch
    uint64_t io_generation_ = 0;                      // bumped by set_source / set_receivers (GraphKey)
    uint64_t source_generation_ = 0, recv_generation_ = 0;  // bumped by set_source / by set_columns (a checkpoint remembers which it saw)
    bool pair_list_early_ok_ = false;             // ensure_pair
    bool pair_unit_waves_ = false;                // the unit list carries each unit's live waves (build_pair_units)
    bool pair_mid_done_ = false, pair_list_done_ = false;  // part A of the pass in flight has served t+1's source / receivers, the list
    int outside_dirty_ = 0;           // steps until the outside nodes are known to be 0 in both fields again
    uint32_t* ref_to_pos_ = nullptr;  // [n_entries] caller's (class offset + boundary_index) -> processing position
    uint8_t* btype_ = nullptr;
    double* fmem_ = nullptr;
    uint32_t* cidx_ = nullptr;
    // boundary entries by plane (build_plane_order; slab path only); `_rest`: without the first n_xw_ entries
    uint32_t* zorder_ = nullptr;
    uint32_t* zorder_rest_ = nullptr;  // (same allocation as zorder_)
    uint32_t* face_order_ = nullptr;   // (same allocation) the entries of a slab's face plane(s)
    uint32_t face_n_ = 0;
    uint32_t* early_order_ = nullptr;  // (same allocation) the entries of the two planes next to each neighbour
    uint32_t early_n_ = 0;
    // a slab's two-step pass with both exchanges under the march (engine_pair.hip.h): planes whose t+1 the march stores
    int pair_s0_ = 0, pair_s1_ = 0;
    bool pair_early_ = false;          // the pass in flight is one (decided in part A, read by part B)
    // time the compute stream spends waiting for ghost planes (wv_enable_kernel_timing on a slab): event pairs around wait_ghosts
    std::vector<hipEvent_t> halo_events_;
    int halo_ev_used_ = 0;
    unsigned halo_timing_calls_ = 0;
    double halo_wait_ms_ = 0;
    uint64_t halo_wait_n_ = 0, early_passes_ = 0;
    // kernel timing of a two-step pass's two boundary launches (part 0: nodes to t+1, part 1: to t+2), in the passes whose march is timed
    // (three-step passes: [2] boundary nodes to t+3, [3] the third level's fix-up list, [4] the three-step march itself -- kept apart
    // from the two-step march's account, a batch may take both kinds of pass)
    static constexpr int kParts = 5;
    std::vector<hipEvent_t> part_events_[kParts];
    int part_ev_used_[kParts] = {0, 0, 0, 0, 0};
    double part_ms_[kParts] = {0, 0, 0, 0, 0};
    uint64_t part_n_[kParts] = {0, 0, 0, 0, 0};
    bool pass_timed_ = false;
    unsigned part_timing_calls_ = 0;
    std::vector<uint32_t> plane_start_, plane_start_rest_;
    // x-facing walls on compact copies in two- and three-step passes (boundary_kernels.hip.h, xwall_node; engine_pair.hip.h)
    uint32_t n_xw_ = 0;            // the first n_xw_ entries qualify (settled with the entry order in init)
    uint32_t* xw_nbr_ = nullptr;   // [4][n_xw_] in-wall neighbours by entry position
    Real* xw_val_ = nullptr;       // [9][n_xw_]: own value at the odd / even level, faced node, level 1's captures; a three-step pass's third generations and level 2's captures
    uint8_t* xw_gok_ = nullptr;    // [n_xw_]: the entry finishes the node behind the one it faces at a three-step pass's third level (xwall_cover_kernel)
    bool xw_built_ = false;        // table and copies allocated (first ensure_pair that may use them)
    bool xw_active_ = false;       // this (mesh, source) runs its passes on them
    bool xw_valid_ = false;        // the copies hold what the fields hold
    uint64_t passes_taken_ = 0;
    // three-step passes (engine_triple.hip.h)
    Real* field1_ = nullptr;           // t+1 at shell and boundary nodes of the pass in flight, zeros at outside nodes
    uint8_t* triple_map_ = nullptr;
    uint32_t* triple_list_ = nullptr;  // third level's fix-up list: every shell node
    uint32_t triple_list_n_ = 0;
    int* suspect_ = nullptr;           // [kRing] per step slot: the march saw an inf / nan
    uint64_t triple_source_ = 0, triple_io_generation_ = ~0ull;
    bool triple_failed_ = false, triple_ready_ = false, triple_attr_set_ = false;
    // the three-step march: its planes (the owned ones, less the face plane and the plane next to it where a neighbour follows), geometry,
    // windows, work list (ensure_triple, build_triple_units)
    wv::MarchPlan triple_plan_;
    uint32_t* triple_units_ = nullptr; // its work list on the device
    bool triple_xw_ = false;           // the passes' three levels take the x-facing walls on their compact copies (and the third-level list leaves the nodes they face out)
    // stored nodes from which the engine takes three-step passes by itself (tools/pass_forms_by_size.py, profiles/r06/pass_forms_by_size_*.txt:
    // Gnode-updates/s two-step / three-step at the end of round 6, fp64: 224^3 187 / 200, 256^3 213 / 243, 320^3 214 / 255, 384^3 267 / 321,
    // 512^3 286 / 362, 768^3 326 / 416, 1024^3 338 / 443; fp32: 384^3 352 / 421, 512^3 487 / 587, 640^3 460 / 484, 768^3 557 / 590,
    // 896^3 536 / 649, 1024^3 626 / 765 -- wherever two-step passes run at all in fp64; in fp32 from the first size measured)
    uint64_t triple_min_nodes_ = sizeof(Real) == 8 ? (12ull << 20) : (24ull << 20);
    int triple_lb_ = 8;                // bytes of a row per lane of the march as set up (triple_lane_bytes)
    // stored row length (elements) from which doubles march on 16-byte lanes (profiles/r06/lane_width_by_size.txt: Gnode-updates/s with
    // 8- / 16-byte lanes 256^3 234 / 226, 320^3 220 / 234, 384^3 281 / 309, 512^3 346 / 340, 768^3 360 / 378, 1024^3 343 / 403)
    int triple_wide_from_ = 320;
    uint64_t triples_taken_ = 0;
    int* status_ = nullptr;
    int* static_flag_dev_ = nullptr;
    int static_flag_ = 0;
    double* coeffs_ = nullptr;
    int* flags_ = nullptr;
    int* flags_host_ = nullptr;
    void* scratch_ = nullptr;
    Real courant_ = 0, courant_sq_ = 0;
    hipStream_t stream_ = nullptr, comm_stream_ = nullptr;
    hipStream_t on_ = nullptr;  // the launch helpers' stream when it is not the compute stream (a slab's face work on its halo stream)
    hipStream_t st() const { return on_ ? on_ : stream_; }
    StreamPlan plan_;
    int tune_variant_ = -1, tune_ry_ = 0, tune_nwx_ = 0, tune_nwy_ = 0, tune_zchunks_ = 0;
    std::vector<hipEvent_t> events_;
    unsigned timing_launches_ = 0;
    int ev_used_ = 0;
    double time_ms_ = 0;
    uint64_t time_n_ = 0;
    // source / receivers
    int source_kind_ = WV_SOURCE_NONE;
    uint64_t source_node_ = 0, signal_len_ = 0, signal_pos_ = 0;
    double* signal_ = nullptr;
    uint64_t* recv_nodes_ = nullptr;
    Real* recv_out_ = nullptr;
    uint32_t n_recv_ = 0;
    uint64_t recv_first_step_ = 0;
    Real* recv_stage_ = nullptr;  // pinned, kRing rows: a copy into pageable memory would make hipMemcpyAsync wait for the stream on the host
    std::vector<double> recv_log_;
    uint64_t wide_gathers_ = 0;        // steps whose receivers took the wide gather (WV_QUERY_WIDE_GATHERS)
    uint64_t graph_wide_gathers_ = 0;  // ... by one replay of the captured batch
    // directional receivers on the device (engine_directional.hip.h): the 7 * n columns are recv_nodes_ / recv_out_ as ever; at the end of
    // a batch the integrator turns the batch's rows into records, and those travel instead of the rows
    struct Directional {
        bool active = false;
        uint32_t n = 0;
        double spacing = 0, k = 0;                 // k = ambient_density * sample_rate
        double* velocity = nullptr;                // device [n][3]
        wv::DirectionalRecord* dev = nullptr;      // device [kRing][n]
        wv_directional_output* host = nullptr;     // page-locked [kRing][n]
        std::vector<wv_directional_output> log;    // records of the completed steps since the receivers were set
        uint64_t generation = 0;                   // bumped whenever the mode is entered or left (a checkpoint remembers which set it saw)
        uint64_t launches = 0;                     // WV_QUERY_DIRECTIONAL_LAUNCHES
    } dir_;
    void directional_release();
    int directional_enqueue(uint64_t batch);
    std::unique_ptr<wv::SlabComm> comm_;
    // the nine plans that accumulate on the device (engine_staged.hip.h)
    enum PlanKind { kSpectrumPlan, kDecayPlan, kIntensityPlan, kArrivalPlan, kLateralPlan, kModulationPlan, kArrivalBandsPlan, kWaterfallPlan, kInterauralPlan, kPlanKinds };
    static constexpr int kPlanBlocks = 2;  // device blocks of accumulated state a plan has at the most
    // wv_checkpoint / wv_rollback (engine_io.hip.h): device copies of the two live fields and the filter memories, and the
    // host-side position that goes with them
    struct Checkpoint {
        Real* field[2] = {nullptr, nullptr};  // [0] current, [1] previous at the time of the save
        double* fmem = nullptr;
        bool valid = false;
        uint64_t steps_done = 0, signal_pos = 0, recv_first_step = 0;
        uint64_t source_generation = 0, recv_generation = 0;  // the source and the receivers in place at the save
        size_t recv_log_size = 0;
        uint32_t n_recv = 0;
        int outside_dirty = 0;
        uint64_t snap_generation = 0, snap_taken = 0, snap_next = 0;  // the snapshot plan's position (engine_snapshot.hip.h)
        double* dir_velocity = nullptr;  // the directional receivers' velocities (engine_directional.hip.h), their log's length, which set
        uint32_t dir_n = 0;              // (receivers the copy has room for)
        size_t dir_log_size = 0;
        uint64_t dir_generation = 0;
        // an accumulating plan's state blocks, count and position (engine_staged.hip.h), by PlanKind; the copies are allocated by the
        // first checkpoint taken under the plan
        struct PlanSave {
            unsigned char* block[kPlanBlocks] = {nullptr, nullptr};
            size_t bytes[kPlanBlocks] = {0, 0};
            uint64_t generation = 0, captures = 0, last_step = 0, next = 0;
        } plan[kPlanKinds];
        void free_plans() {
            for (PlanSave& s : plan)
                for (unsigned char*& block : s.block) {
                    if (block) (void)hipFree(block);
                    block = nullptr;
                }
        }
    } ckpt_;
    // field snapshots (engine_snapshot.hip.h): a ring of device slots the capture kernel fills on the compute stream, each copied to its
    // page-locked twin on a stream of its own, and the log of the snapshots the host holds
    static constexpr int kSnapSlots = 4;
    struct Snapshots {
        bool active = false, wide = false;
        wv_snapshot_plan plan{};
        wv::SnapshotBox box;
        uint64_t generation = 0;        // bumped by every wv_set_snapshots (a checkpoint remembers which plan it saw)
        uint64_t set_at = 0;            // step count when the plan was set
        uint64_t next = wv::kNoSnapshotStep;  // the next snapshot step not yet captured
        uint64_t batch_end = wv::kNoSnapshotStep;  // the snapshot step at which the batch being planned ends at the latest
        uint64_t taken = 0;             // snapshots that reached the held log since the plan was set
        uint64_t first_taken_step = 0;  // the step of snapshot 0
        uint64_t bytes = 0;             // bytes captured
        double kernel_ms = 0;           // capture kernels' time (kernel timing on)
        uint64_t elems = 0;             // floats per snapshot
        int slots = 0, head = 0;        // ring size (2 .. kSnapSlots), the slot the next capture takes
        size_t committed = 0;           // pending captures that are of committed steps (those of earlier batches)
        float* dev[kSnapSlots] = {nullptr, nullptr, nullptr, nullptr};
        float* host[kSnapSlots] = {nullptr, nullptr, nullptr, nullptr};
        hipEvent_t begun[kSnapSlots] = {nullptr, nullptr, nullptr, nullptr};     // before the capture kernel (kernel timing)
        hipEvent_t captured[kSnapSlots] = {nullptr, nullptr, nullptr, nullptr};  // behind it: hands the slot to the copy stream
        hipEvent_t copied[kSnapSlots] = {nullptr, nullptr, nullptr, nullptr};    // the slot is on the host and may be filled again
        bool used[kSnapSlots] = {false, false, false, false}, timed[kSnapSlots] = {false, false, false, false};
        hipStream_t copy_stream = nullptr;
        struct Pending {
            int slot;
            uint64_t step;
        };
        std::deque<Pending> pending;    // captures enqueued, oldest first, not yet in the log
        std::vector<std::vector<float>> spare;  // memory of dropped snapshots, for the next ones
        std::deque<std::pair<uint64_t, std::vector<float>>> held;  // (step, floats), oldest first: snapshots taken - held.size() .. taken - 1
    } snap_;
    static void snapshot_release(Snapshots& s);
    int launch_snapshot_gather(const wv::SnapshotBox& box, bool wide, float* dst);
    int snapshot_capture(uint64_t step);
    int snapshot_harvest(bool wait, size_t limit = ~size_t{0});
    void snapshot_discard_after(uint64_t last_good_step);
    int snapshot_plan_batch();
    int snapshot_begin_run();
    void snapshot_rollback(uint64_t to_step);
    // ---- engine_staged.hip.h: the nine plans that accumulate on the device -- spectrum, decay (plain and banded), intensity, arrival,
    // lateral, modulation, banded arrival, waterfall, interaural -- have ONE life cycle: captures into a device-only stage on the compute stream, committed batch by batch, folded into the
    // plan's accumulated state in one launch when the stage has no slot left, on fetch and on checkpoint.  StagedPlan holds what they
    // share; a plan's own struct adds its wv_*_plan, its tables and what its fold kernel needs
    struct StagedPlan {
        // what the kind is, set once by the plan's own struct
        PlanKind kind;
        const char* name;                   // "spectrum": in "wv_run: the spectrum stage is full" and the like
        const char* setter;                 // "wv_set_spectrum"
        const char* lost;                   // "its sums have": what wv_rollback says of a plan set after the checkpoint
        const char* block_name[kPlanBlocks];  // "the spectrum's sums": what wv_checkpoint has no room for a copy of
        bool host_table;                    // the fold reads a table the host writes: folded_ev is always recorded, and waited on before the table is rewritten
        bool gradients;                     // a capture is intensity_gather_kernel's four planes (timed per slot), not snapshot_gather_kernel's one
        uint64_t max_captures;              // captures the state can count (onsets 32 bits wide, all bits set = none); ~0: no limit
        StagedPlan(PlanKind kind, const char* name, const char* setter, const char* lost, const char* block0, const char* block1, bool host_table,
                   bool gradients, uint64_t max_captures = ~0ull)
            : kind(kind), name(name), setter(setter), lost(lost), block_name{block0, block1}, host_table(host_table), gradients(gradients),
              max_captures(max_captures) {}
        bool active = false;
        bool gather_wide = false;       // the capture takes four nodes per lane (snapshot_plan.h: gather_wide)
        bool fold_wide = false;         // the fold takes two nodes per lane
        wv::SnapshotBox box;
        double spacing = 0;             // of the mesh (gradients only)
        bool ears = false;              // a capture is ear_gather_kernel's two planes (the third kind: neither of the above)
        int32_t ear_a[3] = {0, 0, 0}, ear_b[3] = {0, 0, 0};  // offsets in mesh nodes from a taken node to its ears (ears only)
        uint64_t generation = 0;        // bumped by every call of the setter (a checkpoint remembers which plan it saw)
        wv::CaptureStage st;            // staged steps, committed count, next plan step, the batch's end (capture_stage.h)
        uint64_t nodes = 0;             // B: nodes taken
        float* stage = nullptr;         // [T][B], with gradients [T][4][B]: pressure, gx, gy, gz, with ears [T][2][B]: ear a, ear b
        unsigned char* block[kPlanBlocks] = {nullptr, nullptr};  // the accumulated state: what a checkpoint copies and a rollback restores
        size_t block_bytes[kPlanBlocks] = {0, 0};
        int n_blocks = 0;
        hipEvent_t begun[2] = {nullptr, nullptr};      // before a fold (kernel timing), in turn
        hipEvent_t folded_ev[2] = {nullptr, nullptr};  // behind it; a host table: the host may write the turn's table again
        bool used[2] = {false, false}, timed[2] = {false, false};
        int turn = 0;                   // the event pair (and table) the next fold takes
        uint64_t folds = 0;             // WV_QUERY_*_FOLDS
        double kernel_ms = 0;           // fold kernels' time (kernel timing on)
        hipEvent_t gather_begun[wv::kSpectrumStage] = {}, gather_done[wv::kSpectrumStage] = {};  // around a slot's capture (gradients, kernel timing)
        bool gather_timed[wv::kSpectrumStage] = {};
        double gather_ms = 0;           // capture kernels' time (kernel timing on), over gathers_timed of them
        uint64_t gathers_timed = 0;
    };
    // a table of the staged captures which the host writes into one of two page-locked buffers in turn (two, so that it never rewrites a
    // table a queued copy still reads) and copies ahead of the fold: the bins int32[t] of the decay and the intensity plan (BinTable,
    // engine_decay.hip.h), the twiddles double[t][n_freqs][2] of the spectrum and the modulation plan (TwiddleTable, engine_staged.hip.h);
    // the waterfall plan has one of each
    template <typename T>
    struct HostTable {
        T* host[2] = {nullptr, nullptr};
        T* dev[2] = {nullptr, nullptr};
    };
    using BinTable = HostTable<int32_t>;
    using TwiddleTable = HostTable<double>;
    template <typename T>
    static hipError_t host_table_allocate(HostTable<T>& table, size_t bytes);
    template <typename T>
    static void host_table_free(HostTable<T>& table);
    int bin_table_write(BinTable& table, const StagedPlan& p, int b, int t, uint32_t bin_captures, uint32_t n_bins);
    int twiddle_table_write(TwiddleTable& table, const StagedPlan& p, int b, int t, const std::vector<double>& freqs);
    int fetch_interleaved(const double* re_plane, uint64_t nodes, double* out, std::vector<double>& planes);  // Re, Im planes -> [B][2] on the host
    // the per-node thresholds float[B] of an arrival or a lateral plan: every entry checked, then uploaded beside the candidate's state
    int threshold_map_refused(const char* setter, const float* map, uint64_t nodes);
    hipError_t threshold_map_upload(float*& dev, const float* map, uint64_t nodes);
    // field spectra (engine_spectrum.hip.h): the planar sums the fold kernel accumulates, two twiddle tables (page-locked, and their device
    // copies) the host writes in turn
    struct Spectrum : StagedPlan {
        Spectrum() : StagedPlan(kSpectrumPlan, "spectrum", "wv_set_spectrum", "its sums have", "the spectrum's sums", nullptr, true, false) {}
        wv_spectrum_plan plan{};
        std::vector<double> freqs;      // cycles per step, [K]
        double* acc() const { return reinterpret_cast<double*>(this->block[0]); }  // [K][2][B]
        TwiddleTable tw;
        void free_own() { host_table_free(tw); }
    } spec_;
    int spectrum_enqueue(Spectrum& s, int b, int t, unsigned blocks);
    // energy decay maps (engine_decay.hip.h): the time-binned energies the fold kernel accumulates; a banded plan's filter states and
    // coefficients beside them
    struct Decay : StagedPlan {
        Decay() : StagedPlan(kDecayPlan, "decay", "wv_set_decay", "its bins have", "the decay plan's bins", "the decay plan's filter states", true, false) {}
        wv_decay_plan plan{};
        double* bins() const { return reinterpret_cast<double*>(this->block[0]); }   // [n_bins][B]; a banded plan's: [n_bands][n_bins][B]
        double* state() const { return reinterpret_cast<double*>(this->block[1]); }  // [n_bands][n_sections][2][B]: z1, z2 of every section (banded only)
        uint32_t n_bands = 0, n_sections = 0;  // wv_set_decay_bands: 1 .. 8 cascades of 1 .. 4 sections; 0 = a plain plan
        double* coef = nullptr;         // [n_bands][n_sections][5] on the device (banded only)
        BinTable table;
        void free_own();
    } decay_;
    int decay_set(const wv_decay_plan* plan, const wv_biquad* sections, uint32_t n_bands, uint32_t n_sections, bool banded);
    int decay_fetch(double* dst, uint64_t* captures, bool banded);
    int decay_enqueue(Decay& d, int b, int t, unsigned blocks);
    // intensity maps (engine_intensity.hip.h): the velocities the integrator carries per node and the time-binned sums Ix, Iy, Iz, E the
    // fold kernel accumulates
    struct Intensity : StagedPlan {
        Intensity()
            : StagedPlan(kIntensityPlan, "intensity", "wv_set_intensity", "its bins have", "the intensity plan's bins", "the intensity plan's velocities", true, true) {}
        wv_intensity_plan plan{};
        double k = 0;                   // ambient_density * sample_rate
        double* bins() const { return reinterpret_cast<double*>(this->block[0]); }      // [4][n_bins][B]: Ix, Iy, Iz, E
        double* velocity() const { return reinterpret_cast<double*>(this->block[1]); }  // [3][B]
        BinTable table;
        void free_own();
    } inten_;
    int launch_intensity_gather(const wv::SnapshotBox& box, double spacing, float* dst);  // (engine_snapshot.hip.h, beside launch_snapshot_gather)
    int intensity_enqueue(Intensity& d, int b, int t, unsigned blocks);
    // arrival-aligned energy maps (engine_arrival.hip.h): ONE block of per-node state the fold kernel carries (arrival_plan.h has the
    // places): pre, moment, bins, onset, peak, peak_capture.  The edge table and the number of the first staged capture go to the kernel
    // as arguments: there is no table to copy
    struct Arrival : StagedPlan {
        Arrival() : StagedPlan(kArrivalPlan, "arrival", "wv_set_arrival", "its state has", "the arrival plan's state", nullptr, false, false, wv::kArrivalMaxCaptures) {}
        wv_arrival_plan plan{};
        unsigned char* state() const { return this->block[0]; }  // double pre[B], moment[B], bins[n_bins][B]; uint32 onset[B]; float peak[B]; uint32 peak_capture[B]
        float* threshold_map = nullptr; // [B], or NULL: the plan's scalar for every node
        void free_own();
    } arr_;
    int arrival_enqueue(Arrival& d, int b, int t, unsigned blocks);
    // lateral maps (engine_lateral.hip.h): the intensity plan's stage, and ONE block of per-node state the fold kernel carries
    // (lateral_plan.h has the places): pre, velocity, bins, onset.  No table either
    struct Lateral : StagedPlan {
        Lateral() : StagedPlan(kLateralPlan, "lateral", "wv_set_lateral", "its state has", "the lateral plan's state", nullptr, false, true, wv::kLateralMaxCaptures) {}
        wv_lateral_plan plan{};
        double k = 0;                   // ambient_density * sample_rate
        unsigned char* state() const { return this->block[0]; }  // double pre[B], velocity[3][B], bins[10][n_bins][B]; uint32 onset[B]
        float* threshold_map = nullptr; // [B], or NULL: the plan's scalar for every node
        void free_own();
    } lat_;
    int lateral_enqueue(Lateral& d, int b, int t, unsigned blocks);
    // modulation maps (engine_modulation.hip.h): per band the energy and the Fourier sums of the band-filtered, squared captures at M
    // modulation frequencies, and the filter states beside them; the coefficient table and two twiddle tables (page-locked, and their
    // device copies) the host writes in turn, as the spectrum plan's
    struct Modulation : StagedPlan {
        Modulation()
            : StagedPlan(kModulationPlan, "modulation", "wv_set_modulation", "its sums have", "the modulation plan's sums", "the modulation plan's filter states", true, false) {}
        wv_modulation_plan plan{};
        std::vector<double> freqs;      // cycles per step, [M]
        double* sums() const { return reinterpret_cast<double*>(this->block[0]); }   // [n_bands][1 + 2 M][B]: E, then Re, Im per frequency
        double* state() const { return reinterpret_cast<double*>(this->block[1]); }  // [n_bands][n_sections][2][B]: z1, z2 of every section
        uint32_t n_bands = 0, n_sections = 0;
        double* coef = nullptr;         // [n_bands][n_sections][5] on the device
        TwiddleTable tw;
        void free_own();
    } mod_;
    int modulation_enqueue(Modulation& d, int b, int t, unsigned blocks);
    // band-limited arrival maps (engine_arrival_bands.hip.h): block 0 holds what the fold accumulates (arrival_bands_plan.h has the
    // places): per band pre, moment, bins and a copy of the onset, then peak and peak_capture; block 1 the filter states.  Edges, tail
    // and lags go to the kernel as arguments: there is no table to copy
    struct ArrivalBands : StagedPlan {
        ArrivalBands()
            : StagedPlan(kArrivalBandsPlan, "banded arrival", "wv_set_arrival_bands", "its state has", "the banded arrival plan's sums",
                         "the banded arrival plan's filter states", false, false, wv::kArrivalMaxCaptures) {}
        wv_arrival_bands_plan plan{};
        wv::ArrivalBandsTable table{};  // edges, tail and lags as the kernel takes them
        unsigned char* sums() const { return this->block[0]; }                         // double pre[K][B], moment[K][B], bins[K][n_bins][B]; uint32 onset[K][B]; float peak[B]; uint32 peak_capture[B]
        double* state() const { return reinterpret_cast<double*>(this->block[1]); }  // [n_bands][n_sections][2][B]: z1, z2 of every section
        uint32_t n_bands = 0, n_sections = 0, n_bins = 0;  // n_bins = n_edges + n_tail
        double* coef = nullptr;         // [n_bands][n_sections][5] on the device, and behind it ...
        uint32_t* bin_first() const { return reinterpret_cast<uint32_t*>(coef + (size_t)n_bands * n_sections * wv::kBiquadDoubles); }  // ... [n_bins + 1]: the first rel of every bin, NONE behind the last
        float* threshold_map = nullptr; // [B], or NULL: the plan's scalar for every node
        void free_own();
    } arrb_;
    int arrival_bands_enqueue(ArrivalBands& d, int b, int t, unsigned blocks);
    // waterfall maps (engine_waterfall.hip.h): the planar sums the fold kernel accumulates per time bin and frequency; a bin table AND a
    // twiddle table (each two page-locked buffers and their device copies) the host writes in turn
    struct Waterfall : StagedPlan {
        Waterfall() : StagedPlan(kWaterfallPlan, "waterfall", "wv_set_waterfall", "its sums have", "the waterfall plan's sums", nullptr, true, false) {}
        wv_waterfall_plan plan{};
        std::vector<double> freqs;      // cycles per step, [K]
        double* acc() const { return reinterpret_cast<double*>(this->block[0]); }  // [n_bins][K][2][B]
        BinTable table;
        TwiddleTable tw;
        void free_own() {
            host_table_free(table);
            host_table_free(tw);
        }
    } wf_;
    int waterfall_enqueue(Waterfall& w, int b, int t, unsigned blocks);
    // interaural maps (engine_interaural.hip.h): block 0 holds what a fetch returns (interaural_plan.h has the places): pre, bins, onset;
    // block 1 what only the fold sees: the lag history of both ears and their filter states.  Edges, L and n_sections go to the kernel
    // as arguments: there is no table to copy
    struct Interaural : StagedPlan {
        Interaural()
            : StagedPlan(kInterauralPlan, "interaural", "wv_set_interaural", "its state has", "the interaural plan's sums",
                         "the interaural plan's history and filter states", false, false, wv::kInterauralMaxCaptures) {
            this->ears = true;
        }
        wv_interaural_plan plan{};
        unsigned char* sums() const { return this->block[0]; }   // double pre[2][B], bins[n_bins][2 L + 3][B]; uint32 onset[B]
        unsigned char* carry() const { return this->block[1]; }  // double history[2][L][B], z[2][n_sections][2][B]; null when L == 0 and n_sections == 0
        double* coef = nullptr;         // [n_sections][5] on the device, or NULL: no filter
        float* threshold_map = nullptr; // [B], or NULL: the plan's scalar for every node
        void free_own();
    } ia_;
    int launch_ear_gather(const wv::SnapshotBox& box, const int32_t* ear_a, const int32_t* ear_b, float* dst);  // (engine_snapshot.hip.h, beside the other two)
    int interaural_enqueue(Interaural& d, int b, int t, unsigned blocks);
    // ---- engine_staged.hip.h: one copy of each step of the life cycle
    StagedPlan* const staged_[kPlanKinds] = {&spec_, &decay_, &inten_, &arr_, &lat_, &mod_, &arrb_, &wf_, &ia_};  // by PlanKind
    StagedPlan* staged() const {  // the active one of the nine, or null: they exclude each other (and a snapshot plan)
        for (StagedPlan* p : staged_)
            if (p->active) return p;
        return nullptr;
    }
    enum PlanRow { kSnapshotRow, kSpectrumRow, kBandedDecayRow, kPlainDecayRow, kIntensityRow, kArrivalRow, kLateralRow, kModulationRow, kArrivalBandsRow, kWaterfallRow, kInterauralRow };
    int plan_refused(const std::string& setter, PlanRow self);
    template <typename Plan>
    static void plan_release(Plan& p);
    static void staged_release(StagedPlan& p);
    template <typename Plan>
    int staged_stop(Plan& p);
    hipError_t staged_allocate(StagedPlan& candidate, uint64_t stage_bytes, uint64_t block0_bytes, uint64_t block1_bytes = 0);
    template <typename Plan>
    int staged_install(Plan& current, Plan& candidate, hipError_t rc, const std::string& no_room, uint64_t first_step, uint64_t period);
    int staged_capture(StagedPlan& p, uint64_t step);
    int staged_drain_timing(StagedPlan& p, int turn = -1);
    int staged_fold_begins(StagedPlan& p, int b);
    int staged_enqueue(StagedPlan& p, int b, int t, unsigned blocks);
    int staged_fold(StagedPlan& p);
    int staged_settle(StagedPlan& p);
    enum class PlanTime { folds_ns, gathers_ns, gathers };
    int staged_time_query(StagedPlan& p, PlanTime what, uint64_t* value);
    int staged_plan_batch(StagedPlan& p);
    int staged_begin_run(StagedPlan& p);
    int staged_count(const StagedPlan& p, uint64_t* captures, uint64_t* last_step);
    int staged_checkpoint(StagedPlan& p);
    int staged_rollback(StagedPlan& p);
    // whichever plan is active decides where passes end (engine_batch.hip.h): they all exclude each other
    bool capture_plan_active() const { return snap_.active || staged(); }
    uint64_t capture_next() const { return snap_.active ? snap_.next : staged() ? staged()->st.next : wv::kNoSnapshotStep; }
    uint64_t capture_batch_end() const { return snap_.active ? snap_.batch_end : staged() ? staged()->st.batch_end : wv::kNoSnapshotStep; }
    int capture_step(uint64_t step) { return snap_.active ? snapshot_capture(step) : staged_capture(*staged(), step); }
};

}  // namespace wv
