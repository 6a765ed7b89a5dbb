/*
 * pywindow_amd.h -- C ABI of libpywindow_hip.so, the MI355X (gfx950) engine for
 * pywindow's per-molecule structural analysis.
 *
 * The reference (marcinmiklitz/pywindow) is pure Python and has no FFI layer; the
 * boundary this library stands behind is the set of free functions that
 * src/pywindow/_internal/molecular.py:29-44 imports from utilities.py and that
 * Molecule.full_analysis() chains (molecular.py:156-202).  One *unit* is one
 * (frame, molecule); a batch is every unit of a trajectory, analysed by one
 * kernel launch per GPU.  Each entry point below names the reference function
 * it replaces.
 *
 * Conventions: plain pointers and sizes, caller-allocated buffers, no
 * exceptions across the ABI -- every function returns 0 on success or a
 * negative PW_E_* code.  All arithmetic is IEEE double.  There is no CPU
 * FALLBACK: without a usable HIP device every compute call on a device context
 * fails with PW_E_NO_DEVICE.  (A host context, pw_context_create(-1, ..), is an
 * explicit choice of the caller and runs the same source on host threads.)
 *
 * Threads (the reference's workers are stateless processes,
 * trajectory.py:564-582).  Every entry point that takes a pw_context holds that
 * context's mutex for the duration of the call: any number of threads may call
 * into ONE context, their calls run one after the other, and different contexts
 * share no mutable state -- two threads with a context each (even on the same
 * device) never wait for one another in the library.  pw_last_error() is per
 * thread.  What the library cannot see is which calls belong together.  Three
 * pieces of per-context state outlive a call, and a caller that shares a context
 * between threads keeps each sequence together itself (the Python binding holds
 * Context.lock across them):
 *   - the page-locked staging buffer: pw_context_pinned .. pw_resident_upload
 *     (the buffer is free again when the upload returns);
 *   - "the records fetched last": pw_resident_download / pw_resident_extra_windows
 *     .. pw_context_extra_windows;
 *   - the knobs: pw_context_set_params .. the launches that should see them.
 * pw_history handles are read-only after pw_history_open and may be read from
 * any number of threads; the reader decodes on a team of host threads started
 * once per process, and pw_history_stream_read runs one more thread of its own
 * for the duration of the call (the appends, which take the context's mutex one
 * at a time like any other caller).  A second live device context on a device runs its
 * analyses as single launches (pw_context_pipelined), not as the pipeline.
 */
#ifndef PYWINDOW_AMD_H
#define PYWINDOW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PW_W_MAX 16       /* windows held by the fixed-size record; a molecule with more keeps the first
                             PW_W_MAX there, sets PW_ST_WINDOW_OVERFLOW and hands the rest over through
                             pw_context_extra_windows -- the reference has no limit (utilities.py:1526-1536) */
#define PW_DBSCAN_MAX 8192 /* points pw_dbscan accepts */
#define PW_P_MAX 2048     /* sampling vectors the team workspaces are sized for AT LEAST; the capacity follows
                             the `adjust` knobs of pw_params (the reference's count is unbounded,
                             utilities.py:1409, 1616) and pw_analysis_batch grows it further when a unit asks */

/* error codes */
#define PW_OK 0
#define PW_E_NO_DEVICE (-1)
#define PW_E_BAD_ARG (-2)
#define PW_E_HIP (-3)
#define PW_E_TOO_LARGE (-4) /* a molecule has more atoms than fit in LDS */
#define PW_E_NOMEM (-5)
#define PW_E_RETRY (-6)     /* a capacity was grown for this batch: launch the analysis again, then download */
#define PW_E_TIMEOUT (-7)   /* a launch of the pipeline gave up waiting for another one (pw_last_error names the wait);
                               the records are incomplete: repeat the analysis (pw_context_retries counts repeats).
                               Every wait inside a kernel is bounded by time WITHOUT PROGRESS of the other side:
                               PW_WAIT_LIMIT_MS (default 250) between launches of one analysis -- a window team that sees
                               no unit published, a residency gate that sees no optimiser team start -- and
                               PW_STREAM_LIMIT_MS (default 5000) for the host's next append to a streamed batch; both are
                               read by pw_context_create.  A wait during which the other side keeps making progress (a
                               device shared with another tenant, a batch of long chains) is never cut short. */

/* stage selection bits for pw_analysis_* */
#define PW_STAGE_BASIC 1u   /* molecular_weight, center_of_mass, max_dim, pore_diameter */
#define PW_STAGE_AVG 2u     /* find_average_diameter */
#define PW_STAGE_OPT 4u     /* opt_pore_diameter */
#define PW_STAGE_WINDOWS 8u /* find_windows (implies PW_STAGE_OPT) */
#define PW_STAGE_ALL 15u

/* per-unit status bits (pw_unit_out.status) */
#define PW_ST_OK 0
#define PW_ST_NEGATIVE_PORE 1      /* pore radius <= 0: the reference's bounds would be inverted */
#define PW_ST_WINDOW_OVERFLOW 2    /* more than PW_W_MAX windows: n_windows is the true count, the record holds the
                                      first PW_W_MAX, the others are in the context's extra-window list */
#define PW_ST_POINTS_OVERFLOW 4    /* more sampling vectors than the workspace of this launch holds (n_points /
                                      n_points_avg say how many): avg_d is NaN / n_windows -1, NOT a result */
#define PW_ST_WINDOW_DROPPED 8     /* a cluster's refined path scan failed (reference: None + warning) */
#define PW_ST_WINDOW_NEGATIVE 16   /* a window diameter < 0 (reference: warning) */
#define PW_ST_Z_BOUNDS 32          /* z_bounds upper < -new_z with lb_z (reference: scipy raises ValueError) */
#define PW_ST_TOO_FEW_POINTS 64    /* fewer than 10 sampling vectors in find_windows (reference: KDTree.query(k=10)
                                      raises ValueError, utilities.py:1428-1431) */
#define PW_ST_PATH_TOO_LONG 128    /* find_windows: a sampling vector's path would have more than 2^20 points (sphere radius /
                                      increment, or / increment2): a pore centre that an open or enormous search box let run
                                      away.  The reference builds such a path as a Python list (MemoryError, or hours);
                                      no windows are computed for the unit */

/* Input batch: ragged molecules, atoms of unit u are [atom_offset[u], atom_offset[u+1]). */
typedef struct pw_batch_in {
    int64_t n_units;
    const int64_t *atom_offset; /* n_units + 1 */
    const double *xyz;          /* sum(N) x 3, row-major as numpy (N,3) */
    const double *vdw;          /* per atom: atomic_vdw_radius[element] (tables.py:111-197) */
    const double *mass;         /* per atom: atomic_mass[element]      (tables.py:22-108)  */
    int64_t template_atoms;     /* 0: vdw / mass have one entry per atom of the batch (sum(N));
                                   T > 0: every unit has T atoms and vdw / mass are ONE template of T
                                   entries -- the frames of a trajectory share their elements
                                   (trajectory.py:245-248), so the constants travel once */
} pw_batch_in;

/* Fixed-size result record of one unit == Molecule.properties (molecular.py:215-352). */
typedef struct pw_unit_out {
    int32_t n_atoms;
    int32_t status;
    double mw;             /* molecular_weight()        utilities.py:96  */
    double com[3];         /* center_of_mass()          utilities.py:127 */
    double maxd;           /* max_dim()                 utilities.py:355 */
    int32_t maxd_i, maxd_j;
    double avg_d;          /* find_average_diameter()   utilities.py:1586 */
    double pore_d;         /* pore_diameter()           utilities.py:375 */
    int32_t pore_atom;
    int32_t pore_opt_atom;
    double pore_vol;       /* sphere_volume(pore_d/2)   utilities.py:429 */
    double pore_opt_d;     /* opt_pore_diameter()       utilities.py:400 */
    double pore_opt_c[3];
    double pore_vol_opt;
    int32_t n_windows;     /* find_windows(): -1 => None, else number of windows  utilities.py:1364 */
    int32_t n_clusters;
    double win_d[PW_W_MAX];
    double win_c[PW_W_MAX][3];
    /* diagnostics (not part of the reference's dict; used by the parity tests) */
    int32_t n_points;      /* sampling vectors in find_windows */
    int32_t n_points_avg;  /* sampling vectors in find_average_diameter */
    int32_t n_survivors;   /* vectors that reach the outside */
    int32_t opt_nit, opt_nfev, opt_task, opt_msg;
    int32_t n_eval;        /* point-vs-molecule evaluations performed */
    double eps;            /* DBSCAN radius */
    double sphere_r;       /* sampling sphere radius in find_windows */
} pw_unit_out;

/* A window beyond the PW_W_MAX the record holds (PW_ST_WINDOW_OVERFLOW): position `index` >= PW_W_MAX in
 * the reference's output order of unit `unit` (utilities.py:1526-1536). */
typedef struct pw_extra_window {
    int64_t unit;
    int32_t index;
    int32_t reserved;
    double d;
    double c[3];
} pw_extra_window;

/* Stage-level capture of find_windows for one unit (pw_analysis_debug; the parity tests compare it
 * with the reference's intermediate results). */
typedef struct pw_unit_debug {
    int32_t n_survivors;            /* sampling vectors that pass vector_analysis (utilities.py:1457-1467) */
    int32_t n_clusters;
    int32_t pass_idx[PW_P_MAX];     /* their indices on the sampling sphere, ascending (the first PW_P_MAX) */
    int32_t labels[PW_P_MAX];       /* DBSCAN label of each (utilities.py:1478-1487) */
    double gap2[PW_P_MAX];          /* vector_analysis result [1]: 2 * narrowest gap along the path */
    double win[PW_W_MAX][12];       /* window_analysis per cluster (utilities.py:1191-1361): chosen vector (3),
                                       angle_1, angle_2 (as angle_between_vectors returns them), new_z,
                                       diameter at the neck point, z optimum,
                                       x, y optimum, final diameter, evaluations */
} pw_unit_debug;

/* Optional knobs of the reference's free functions.  Defaults are the
 * values Molecule.full_analysis() uses; a context starts with the defaults. */
typedef struct pw_params {
    double adjust_windows;  /* find_windows(adjust=1):           sampling density, utilities.py:1410 */
    double adjust_average;  /* find_average_diameter(adjust=1):  sampling density, utilities.py:1615 */
    double increment;       /* find_windows(increment=1.0):      coarse path-scan step, utilities.py:1457 */
    int32_t pore_opt;       /* find_windows(pore_opt=True): centre on the optimised pore, :1380-1393 */
    int32_t opt_flags;      /* opt_pore_diameter(bounds=, com=), utilities.py:400-426: PW_OPT_* bits */
    double opt_x0[3];       /* com=: start of the optimisation (default: the centre of mass) */
    double opt_lo[3];       /* bounds=: lower / upper bound per axis, -/+HUGE_VAL for None */
    double opt_hi[3];       /*          (default: start -/+ the pore radius at the start) */
    /* window_analysis(increment2=0.1, z_bounds=None, lb_z=True, z_second_mini=False), utilities.py:1191-1200 */
    double increment2;      /* refined path-scan step along the chosen vector, :1221-1224 */
    double z_lo, z_hi;      /* z_bounds: -/+HUGE_VAL for None; z_lo is replaced by -new_z when lb_z, :1296-1297 */
    int32_t lb_z;           /* lower bound of the neck search = -new_z (default 1) */
    int32_t z_second_mini;  /* second neck search after the in-plane optimisation, :1326-1334 (default 0) */
} pw_params;
#define PW_OPT_CUSTOM_START 1
#define PW_OPT_CUSTOM_BOUNDS 2

typedef struct pw_context pw_context;   /* device, stream, workspace */
typedef struct pw_resident pw_resident; /* a batch resident in HBM */

int pw_device_count(void);
const char *pw_version(void);
const char *pw_last_error(void);

/* device >= 0: a HIP device ordinal.  device == -1: the explicit HOST path -- the same unit pipeline
 * (pywindow_amd/csrc/pw_unit.hpp, single source with the kernels) compiled for the host and run by threads
 * over the units; it serves pw_analysis_batch / pw_analysis_debug / pw_point_gaps and the pw_resident_*
 * calls (batches then live in host memory), nothing else, and it is never chosen implicitly: a context
 * for a device that does not exist fails with PW_E_NO_DEVICE.  (BASELINE.json configs[0].) */
int pw_context_create(int device, pw_context **ctx);
/* Page-locked host staging buffer owned by the context (at least `bytes`, valid until a later call asks
 * for more): a reader that decodes frames straight into it (pw_history_read) makes the copies of
 * pw_resident_upload asynchronous DMA.  Device contexts only. */
int pw_context_pinned(pw_context *ctx, size_t bytes, void **ptr);
/* threads of a device == -1 context (default: PW_CPU_THREADS or the hardware concurrency); threads <= 0
 * only reports.  Returns 0 for device contexts. */
int pw_context_host_threads(pw_context *ctx, int threads);
void pw_context_destroy(pw_context *ctx);
/* knobs used by every later launch on this context (validated: adjust > 0, increment > 0) */
void pw_params_default(pw_params *params);
int pw_context_set_params(pw_context *ctx, const pw_params *params);

/* Host-buffer path: H2D copy, one launch, D2H copy, synchronous.
 * Replaces the per-frame loop `mol.full_analysis()` of trajectory.py:518-522
 * for `stages == PW_STAGE_ALL`; partial `stages` give the fine-grained calls
 * (pore_diameter, max_dim, ... ) the parity tests exercise one by one. */
int pw_analysis_batch(pw_context *ctx, const pw_batch_in *in, uint32_t stages, pw_unit_out *out);
/* Windows beyond PW_W_MAX of the analysis whose records were fetched last on this context
 * (pw_analysis_batch, pw_analysis_debug, pw_resident_download), ordered by (unit, index): copies at
 * most `cap` entries to buf and returns how many exist.  find_windows has no upper limit on the
 * number of windows (utilities.py:1526-1536); the record keeps the first PW_W_MAX. */
int64_t pw_context_extra_windows(pw_context *ctx, pw_extra_window *buf, int64_t cap);
/* 1 when analyses on this context run as the overlapped two-launch pipeline (optimiser chains | average diameter + window search), 0 when as single launches:
 * the pipeline needs its ten HIP streams to run concurrently, i.e. GPU_MAX_HW_QUEUES >= 10 in the
 * environment BEFORE the process first initialises HIP; pw_context_create measures whether they do and
 * falls back (with a line on stderr) instead of letting gate kernels wait for launches queued behind them */
int pw_context_pipelined(pw_context *ctx);
/* diagnostic: how many gates of the pipeline gave up waiting since the context was created (tail gates |
 * head gates << 16 | residency gates << 32).  Tail and head gates only pace launches: an expiry costs 20 ms and
 * changes no result.  A residency gate that sees no optimiser team start for PW_WAIT_LIMIT_MS lets the launches
 * behind it go when some teams HAVE started (the device is busy; nothing is lost) and gives the analysis up
 * (PW_E_TIMEOUT) when not one has.  Zero on a healthy device. */
int pw_context_gate_timeouts(pw_context *ctx, uint64_t *count);
/* How many analyses were REPEATED on this context after a launch gave up waiting for another one (PW_E_TIMEOUT):
 * by pw_analysis_batch / pw_analysis_debug themselves (up to PW_TIMEOUT_REPEATS times, default 2), and by callers of the pw_resident_*
 * entry points, who repeat on PW_E_TIMEOUT and say so with pw_context_count_retry.  Zero on a healthy device;
 * pw_retries_total() is the same over every context of the process.  (The reference has nothing to compare:
 * its Pool workers either return or raise, trajectory.py:553-586.) */
int pw_context_retries(pw_context *ctx, uint64_t *count);
int pw_context_count_retry(pw_context *ctx);
uint64_t pw_retries_total(void);
/* diagnostic: the hand-off queues of the pipeline's sets as they are now -- out[4 * s + 0..3] = units taken by
 * window teams (head), published by optimiser chains (tail), optimiser teams started, error flag of set s;
 * s < 4 (cap >= 16).  Reads device memory without waiting for anything. */
int pw_context_queue_state(pw_context *ctx, uint64_t *out, int cap);
/* sampling vectors the team workspaces of this context currently hold per molecule (>= PW_P_MAX) */
int pw_context_point_capacity(pw_context *ctx);
/* at least n_points sampling vectors per molecule in the workspaces of every later launch.  pw_analysis_batch
 * does this by itself when a unit carries PW_ST_POINTS_OVERFLOW (the reference's count
 * int(log10(4 pi R^2) * 250 * adjust), utilities.py:1409, 1616, has no upper limit); callers of the
 * pw_resident_* entry points read n_points / n_points_avg of the flagged records, reserve, launch again. */
int pw_context_reserve_points(pw_context *ctx, int64_t n_points);

/* A batch of ONE molecule type whose coordinates arrive in pieces, in unit order, while it is being analysed
 * (the frame loop of the reference reads and analyses frame after frame, trajectory.py:496-522; here the reader
 * feeds a launch that is already running).  begin: sizes known, radii / masses as a template of template_atoms
 * entries; pw_resident_launch may follow at once -- the launch's teams wait for the units they are handed.
 * append: coordinates [count][template_atoms][3] of units first .. first + count - 1, `first` = the number appended
 * so far; the call returns when the copy has landed (from page-locked memory, pw_context_pinned, a DMA of tens of
 * microseconds per megabyte) and the buffer may be reused.  Downloading an incomplete batch is PW_E_BAD_ARG; a
 * launch that sees no unit appended for PW_STREAM_LIMIT_MS (5 s) gives up and the download reports it (PW_E_TIMEOUT).  Device contexts only;
 * molecules beyond LDS (PW_E_TOO_LARGE) go through pw_resident_upload.  On a context that runs an analysis as ONE
 * launch (pw_context_pipelined() == 0), or for stages without the window search, a launch asked for before the last
 * unit has arrived is made by the append that completes the batch (nothing overlaps, nothing waits). */
int pw_resident_stream_begin(pw_context *ctx, int64_t n_units, int64_t template_atoms, const double *vdw,
                             const double *mass, pw_resident **res);
int pw_resident_stream_append(pw_context *ctx, pw_resident *res, const double *xyz, int64_t first, int64_t count);

/* The same analysis with the intermediate results of find_windows captured per unit (dbg: n_units
 * records, caller-allocated).  Test instrumentation: one launch at a time, no overlap. */
int pw_analysis_debug(pw_context *ctx, const pw_batch_in *in, uint32_t stages, pw_unit_out *out,
                      pw_unit_debug *dbg);

/* Fine-grained: min_i(|r_i - p| - vdw_i) and its first argmin at arbitrary points,
 * point q belonging to unit unit_of_point[q]  (pore_diameter(.., com=p)[0]/2 and [1],
 * utilities.py:375-388; the objective of every optimiser on the path). */
int pw_point_gaps(pw_context *ctx, const pw_batch_in *in, const int64_t *unit_of_point,
                  const double *points, int64_t n_points, double *gap, int32_t *argmin);

/* Fine-grained: sklearn.cluster.DBSCAN(eps, min_samples=5).fit(points).labels_ as find_windows calls it
 * (utilities.py:1478-1487; sklearn/cluster/_dbscan_inner.pyx): clusters numbered in the order of their
 * smallest member, border points with the lowest-numbered adjacent cluster, noise -1.  n <= PW_DBSCAN_MAX points
 * (n x 3, row-major).  mode bit 0: a one-wave team instead of four waves; bit 1: every array of the routine
 * in global memory instead of LDS. */
int pw_dbscan(pw_context *ctx, const double *points, int64_t n, double eps, int mode, int32_t *labels,
              int32_t *n_clusters);

/* Fine-grained: numpy's float64 add.reduce over a contiguous array (pairwise blocks of <= 128 with eight
 * accumulators, 8192-element buffers) as one team computes it -- the order behind np.mean / np.sum in
 * utilities.py:1434 (mean of the k-NN distances) and :1650 (mean of the ray exits).  mode bit 0: a
 * one-wave team instead of four waves; bit 1: the team's scratch in global memory instead of LDS. */
int pw_pairwise_sum(pw_context *ctx, const double *values, int64_t n, int mode, double *sum);

/* Resident path (inputs stay in HBM between launches; used by bench.py and the
 * trajectory driver when several analyses run on the same frames). */
int pw_resident_upload(pw_context *ctx, const pw_batch_in *in, pw_resident **res);
int pw_resident_launch(pw_context *ctx, pw_resident *res, uint32_t stages); /* async on ctx stream */
int pw_resident_sync(pw_context *ctx);
int pw_resident_download(pw_context *ctx, pw_resident *res, pw_unit_out *out);
void pw_resident_free(pw_context *ctx, pw_resident *res);
/* `iters` back-to-back launches bracketed by HIP events on the launch stream;
 * writes the average milliseconds per launch. */
int pw_resident_time(pw_context *ctx, pw_resident *res, uint32_t stages, int iters, float *ms_per_launch);
/* one analysis on its own, timed per launch of the pipeline with HIP events on the launch's own
 * stream: ms[0] optimiser chains, ms[1] always 0 (the average diameter runs inside the window teams),
 * ms[2] average diameter and window search (measurement only) */
int pw_resident_stage_times(pw_context *ctx, pw_resident *res, float *ms3);
/* raw device pointer of the result records (for RCCL gathers by the host side) */
void *pw_resident_device_results(pw_resident *res);
/* For callers that read the records on the device (pw_resident_results_ready): waits for the latest
 * launch of the batch, fails with PW_E_TIMEOUT if its window launch timed out, and loads its windows beyond
 * PW_W_MAX into the context's list (*count of them; pw_context_extra_windows reads them).  PW_E_RETRY: the
 * device list for them has just been allocated -- launch again.  pw_resident_download does all of this. */
int pw_resident_extra_windows(pw_context *ctx, pw_resident *res, int64_t *count);
/* Stream-ordered hand-over of the latest launch's records to a stream of the caller (hipStream_t as
 * an opaque pointer; NULL = the legacy default stream): work queued on `stream` afterwards sees the
 * finished records at *results (device pointer), without a host synchronisation.  This is how the
 * one collective of a multi-GPU run -- the gather of the records, Trajectory._analysis_parallel's
 * pool.get() (trajectory.py:553-586) -- reads them: no host bounce. */
int pw_resident_results_ready(pw_context *ctx, pw_resident *res, void *stream, void **results);
/* ... and the way back: the launch that next overwrites those records waits for everything queued
 * on `stream` so far (call it after queueing the gather). */
int pw_resident_results_release(pw_context *ctx, pw_resident *res, void *stream);
int64_t pw_resident_units(pw_resident *res);
/* the HIP stream (hipStream_t) launches are issued on, as an opaque pointer */
void *pw_context_stream(pw_context *ctx);

/* ---- periodic pre-processing ---------------------------------------------
 * create_supercell (utilities.py:768-810) + discrete_molecules (utilities.py:820-1085) as
 * driven by MolecularSystem.rebuild_system / make_modular (molecular.py:672-708, 798-824):
 * split every frame of a system into discrete molecules; with `rebuild`, molecules wrapped
 * across the cell faces are re-assembled from the 3x3x3 supercell and the copies whose
 * centre of mass lies outside the cell are dropped.  Atom order inside each molecule and
 * the order of the molecules are the reference's.  One topology (covalent radii, masses,
 * terminal flags) for all frames; coordinates and lattice per frame. */
typedef struct pw_cell_in {
    int64_t n_frames;
    int32_t n_atoms;           /* atoms per frame */
    int32_t rebuild;           /* 1: rebuild through the periodic boundary (needs lattice) */
    const double *xyz;         /* n_frames x n_atoms x 3, as loaded (not rounded) */
    const double *lattice;     /* n_frames x 9 row-major lattice matrices; NULL = non-periodic */
    const double *lattice_inv; /* n_frames x 9: numpy.linalg.inv(lattice), utilities.py:726 */
    const double *cov;         /* n_atoms: atomic_covalent_radius[element] (tables.py:200-286) */
    const double *mass;        /* n_atoms */
    const uint8_t *terminal;   /* n_atoms: 1 if the element ends a bond path (utilities.py:943) */
    double max_dist;           /* 2 * max covalent radius present + tol (utilities.py:949-953) */
    double tol;                /* bond tolerance, 0.4 */
} pw_cell_in;

#define PW_RB_NB_CAP 16         /* candidates kept per atom (csrc/pw_rebuild.hpp: RB_NB_CAP) */
#define PW_RB_NB_OVERFLOW 1     /* more than PW_RB_NB_CAP candidate partners of one atom: (image, atom) pairs inside
                                   max_dist and the pair's own bond range, with 2e-3 and rounding to spare */
#define PW_RB_SEG_OVERFLOW 2    /* more than 2 * PW_RB_NB_CAP hits of one atom in one layer: cannot be raised */
#define PW_RB_ATOMS_OVERFLOW 4  /* atoms_cap too small (retry with a larger one) */
#define PW_RB_MOLS_OVERFLOW 8   /* mols_cap too small */
#define PW_RB_THIN_CELL 16      /* a perpendicular height of the cell, V / |b x c|, is below max_dist */

typedef struct pw_cell_out {   /* caller-allocated */
    int32_t atoms_cap;         /* output atoms per frame */
    int32_t mols_cap;          /* output molecules per frame */
    int32_t *n_mol;            /* n_frames */
    int32_t *status;           /* n_frames: PW_RB_* bits */
    int32_t *mol_offset;       /* n_frames x (mols_cap + 1): atoms of molecule m are [off[m], off[m+1]) */
    int32_t *src_atom;         /* n_frames x atoms_cap: index of the input atom */
    int8_t *src_image;         /* n_frames x atoms_cap: -1 = the input atom itself, else image 0..26
                                  (a, b, c nested, 13 = the cell) */
    double *xyz;               /* n_frames x atoms_cap x 3: coordinates rounded to 8 decimals */
} pw_cell_out;

int pw_discrete_molecules(pw_context *ctx, const pw_cell_in *in, const pw_cell_out *out);
/* The same, but the molecules of all frames stay on the device as ONE resident batch (units in
 * frame order, then molecule order) ready for pw_resident_launch: the modular branch of
 * Trajectory._analysis_serial (trajectory.py:512-522) without a host round trip.  `vdw`: van der
 * Waals radius per input atom.  n_mol / status (n_frames each) are returned to the host; *res is
 * NULL when no frame has a molecule.  PW_E_TOO_LARGE: a frame needs larger caps (retry). */
int pw_resident_from_cells(pw_context *ctx, const pw_cell_in *in, const double *vdw, int32_t atoms_cap,
                           int32_t mols_cap, pw_resident **res, int32_t *n_mol, int32_t *status);
int pw_context_device(pw_context *ctx);

/* ---- shape descriptors and circumcircles --------------------------------------
 * get_gyration_tensor / get_inertia_tensor / get_tensor_eigenvalues(sort=True) / calc_asphericity /
 * calc_acylidricity / calc_relative_shape_anisotropy (utilities.py:434-650) of every unit of a batch
 * in one launch.  The tensors are bit-identical to the reference's (numpy's summation orders are
 * reproduced, including the N x N broadcast of utilities.py:511-522); the eigenvalues come from a
 * Jacobi iteration instead of LAPACK dgeev and agree to a few ulps of the largest one. */
typedef struct pw_shape_out {
    double gyration[3][3];
    double inertia[3][3];
    double eigenvalues[3];             /* of the inertia tensor, descending */
    double asphericity;
    double acylidricity;
    double relative_shape_anisotropy;
} pw_shape_out;
int pw_shape_batch(pw_context *ctx, const pw_batch_in *in, pw_shape_out *out);
/* circumcircle(coordinates, atom_sets) (utilities.py:1653-1691) for one molecule: n_sets triples of
 * atom indices -> diameters (n_sets) and centres (n_sets x 3). */
int pw_circumcircle(pw_context *ctx, const double *xyz, int64_t n_atoms, const int32_t *atom_sets,
                    int64_t n_sets, double *diameter, double *centre);

/* ---- distributions of analysis results: Gaussian kernel density sums -----------------------------
 * What the reference's trajectory examples do with the analysis (examples/example_7.py:55-80): the
 * window / pore / maximum diameters of a trajectory go through scipy.stats.gaussian_kde on a grid.
 * One call takes n_jobs independent jobs (the per-molecule curves of a modular trajectory are many
 * small ones); job k has samples x = samples[sample_first .. +n_samples), points
 * g = points[point_first .. +n_points) and writes the RAW sums
 *     sums[point_first + j] = sum_i exp(-0.5 * ((g[j] - x[i]) * inv_bandwidth)^2)
 * The normalisation 1 / (n h sqrt(2 pi)) is the caller's, so that sums of parts of a sample set add.
 * inv_bandwidth is 1 / h as a double the caller computed once; the product by it IS the definition
 * (no division is repeated here).  The result is defined to the bit (pywindow_amd/csrc/pw_kde.hpp):
 * the project's own exp (pw_math.hpp: pw_exp, within 1 ulp, results below the smallest normal are zero),
 * partial sums over chunks of 512 samples added in order, the chunks' sums added in chunk order -- the
 * same on every device, launch geometry, run, and on a device == -1 context (host threads).
 * All pointers are host memory.  A job without samples gives zeros; jobs may share samples and points
 * but not entries of `sums`.  inv_bandwidth <= 0, or a NaN or infinity in it, the samples or the points
 * of any job: PW_E_BAD_ARG (pw_last_error names the job), and nothing is launched or written.
 * Device work is queued on the context's stream; the call returns when the sums are in place. */
typedef struct pw_kde_job {
    int64_t sample_first, n_samples;   /* into `samples` */
    int64_t point_first, n_points;     /* into `points` and `sums` */
    double inv_bandwidth;              /* 1 / h, h the standard deviation of the kernel */
} pw_kde_job;
int pw_kde_sums(pw_context *ctx, const pw_kde_job *jobs, int64_t n_jobs, const double *samples,
                const double *points, double *sums);
/* The joint distribution of TWO quantities (how the pore moves with the windows over a trajectory): what
 * scipy.stats.gaussian_kde does with a 2 x n dataset and a mesh of points.  With a full covariance the
 * kernel does not factor into two one-dimensional sums, hence an entry of its own.  samples and points
 * are arrays of PAIRS ([.][2]: entry i is samples[2 i], samples[2 i + 1]); sample_first, n_samples,
 * point_first, n_points count pairs; sums has one double per point.  Job k writes the RAW sums
 *     sums[point_first + j] = sum_i exp(-0.5 * (z0^2 + z1^2)),
 *     z0 = dx * w00,  z1 = dx * w10 + dy * w11,  (dx, dy) = point j - sample i
 * where w00, w10, w11 are the lower-triangular inverse of the Cholesky factor L of the kernel's covariance
 * (w00 = 1 / l00, w10 = -l10 / (l00 l11), w11 = 1 / l11), three doubles the caller computed once; the caller
 * divides by n * 2 pi * l00 * l11.  Defined to the bit like pw_kde_sums (pw_kde.hpp: the difference is taken
 * first and whitened second, z1 and z0^2 + z1^2 are single fused multiply-adds, the same pw_exp, the same
 * chunks of 512 samples in the same order) -- the same on every device, launch geometry, run and on a
 * device == -1 context; the partial sums of one call stay within a fixed workspace (64 MiB) whatever the
 * size of the mesh, and the result does not depend on how the mesh was cut to achieve that.
 * All pointers are host memory.  A job without samples gives zeros; jobs may share samples and points but
 * not entries of `sums`.  w00 <= 0, w11 <= 0, or a NaN or infinity in the three factors, the samples or the
 * points of any job: PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is launched or
 * written.  Device work is queued on the context's stream; the call returns when the sums are in place. */
typedef struct pw_kde2_job {
    int64_t sample_first, n_samples;   /* pairs, into `samples` */
    int64_t point_first, n_points;     /* pairs, into `points`; entries of `sums` */
    double w00, w10, w11;              /* inverse of the Cholesky factor of the kernel's covariance */
} pw_kde2_job;
int pw_kde2_sums(pw_context *ctx, const pw_kde2_job *jobs, int64_t n_jobs, const double *samples,
                 const double *points, double *sums);
/* The one-dimensional sums under MANY weight vectors at once: scipy.stats.gaussian_kde(samples, bw_method,
 * weights=w) for a reweighted run, and the replicas of a block bootstrap (a replica is the sample set with integer
 * multiplicities) for an error band.  All replicas share every exponential.  Job k has samples
 * x = samples[sample_first .. +n_samples), points g = points[point_first .. +n_points), n_replicas weight
 * vectors laid out sample-major, w[i][b] = weights[weight_first + i * n_replicas + b], and writes, replica-major,
 *     sums[out_first + b * n_points + j] = sum_i w[i][b] * exp(-0.5 * ((g[j] - x[i]) * inv_bandwidth)^2)
 * The caller divides by sum_i w[i][b] * h * sqrt(2 pi).  Defined to the bit (pw_kde.hpp): the terms are
 * pw_kde_sums' own, a chunk of 512 samples is accumulated by fused multiply-adds p = fma(w, term, p) from +0 in
 * sample order, the chunks' sums are added in chunk order -- the same on every device, launch geometry, run and
 * on a device == -1 context; a replica's sums do not depend on which other replicas its job carries, and with
 * all weights 1.0 they are pw_kde_sums' bits.  The partial sums of one call stay within a fixed workspace
 * (64 MiB) and the result does not depend on how points and replicas were cut to achieve that.
 * All pointers are host memory.  A job without samples writes zeros, a job without points nothing; jobs may
 * share samples, points and weights but not entries of `sums`.  n_replicas < 1, inv_bandwidth <= 0, a negative
 * weight, or a NaN or infinity in inv_bandwidth, the samples, the points or the weights of any job:
 * PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is launched or written.  Device work
 * is queued on the context's stream, its memory allocated and freed in stream order; the call returns when
 * the sums are in place. */
typedef struct pw_kdew_job {
    int64_t n_samples, n_points, n_replicas;
    int64_t sample_first, point_first;   /* into `samples` / `points`, as pw_kde_job */
    int64_t weight_first;                /* into `weights`: w[i * n_replicas + b], sample-major */
    int64_t out_first;                   /* into `sums`:    S[b * n_points + j], replica-major */
    double inv_bandwidth;                /* 1 / h */
} pw_kdew_job;
int pw_kde_wsums(pw_context *ctx, const pw_kdew_job *jobs, int64_t n_jobs, const double *samples,
                 const double *points, const double *weights, double *sums);
/* ---- dynamics of analysis results: lagged sums of a time correlation ------------------------------------
 * How long a value of a trajectory lasts and whether one quantity follows another: the raw sums of an auto-
 * or cross-correlation over the frame axis.  The reference has no counterpart (its examples stop at the
 * distributions above).  Job k has two series a = series[a_first .. +n), b = series[b_first .. +n) -- the
 * same range for an autocorrelation -- and writes, for lag j = 0 .. n_lags - 1,
 *     sums[out_first + j] = sum over t in [0, n - j) of a[t] * b[t + j]
 * Negative lags are the caller's (swap a and b).  The entry knows nothing of means, gaps or normalisation:
 * the caller hands over centred series with zeros in the gaps, and gets the number of valid pairs of a lag
 * from a second job over the two 0/1 masks (sums of ones are exact), so that sums of parts add.
 * Defined to the bit (pywindow_amd/csrc/pw_corr.hpp): the t axis is cut into chunks of 512 from t = 0
 * whatever the lag, a chunk's terms are accumulated by fused multiply-adds from zero in t order, the chunks'
 * sums are added in chunk order -- the same on every device, launch geometry, run and on a device == -1
 * context (host threads); the partial sums of one call stay within a fixed workspace (64 MiB) whatever the
 * number of lags, and the result does not depend on how the lags were cut to achieve that.
 * All pointers are host memory.  Any mix of job sizes in one call; a job with n == 0 writes nothing; jobs may
 * share entries of `series` but not of `sums`.  n_lags > n, n_lags < 1 with n > 0, or a NaN or infinity in a
 * series a job reads: PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is launched or
 * written.  Device work is queued on the context's stream, its memory allocated and freed in stream order;
 * the call returns when the sums are in place. */
typedef struct pw_corr_job {
    int64_t a_first, b_first, n;       /* into `series`; a and b may be the same range */
    int64_t out_first, n_lags;         /* into `sums`; 1 <= n_lags <= n */
} pw_corr_job;
int pw_corr_sums(pw_context *ctx, const pw_corr_job *jobs, int64_t n_jobs, const double *series, double *sums);
/* ---- spectra of analysis results: sums of a series against cosines and sines at rational frequencies ----
 * At which frequency a cage breathes: the raw sums of a (Lomb-Scargle) periodogram over the frame axis.  The
 * reference has no counterpart.  Job k has a series a = series[a_first .. +n), a period M and n_freq integer
 * numerators j_q = j_first + q * j_step -- frequency j_q / M cycles per sample -- and writes, for q < n_freq,
 *     re[out_first + q] = sum over t in [0, n) of a[t] cos(2 pi j_q t / M)
 *     im[out_first + q] = sum over t in [0, n) of a[t] sin(2 pi j_q t / M)
 * The entry knows nothing of means, gaps or normalisation: the caller hands over a centred series with zeros
 * in the gaps and transforms the 0/1 mask with further jobs (at j and at 2 j: j_step = 2).
 * Defined to the bit (pywindow_amd/csrc/pw_dft.hpp): the phase of an integer k is q = (j k) mod M in 64-bit
 * integers, folded to q - M when 2 q >= M, u = (double)q / (double)M, ang = u * 6.283185307179586, and its
 * (sine, cosine) pw_sincos(ang) -- the phases are exact integers, so the angle never exceeds pi.  The t axis is
 * cut into chunks of 512 from t = 0; inside chunk ch, with r = t - 512 ch and (cA, sA) the phase of k = r,
 * pc = fma(a[t], cA[r], pc) and ps = fma(a[t], sA[r], ps) from +0 in r order; with (cB, sB) the phase of
 * k = 512 ch, re_ch = fma(cB, pc, -(sB * ps)) and im_ch = fma(sB, pc, cB * ps); the re_ch / im_ch are added in
 * chunk order from +0 -- the same on every device, launch geometry, run and on a device == -1 context (host
 * threads), whatever else shares the call; twiddles and partial sums of one call stay within a fixed workspace
 * (64 MiB) whatever the number of frequencies, and the result does not depend on how they were cut for that.
 * All pointers are host memory.  Any mix of job sizes in one call; a job with n == 0 or n_freq == 0 writes
 * nothing; jobs may share entries of `series` but not of `re` / `im`.  n > 2^31, a period outside 2 .. 2^31,
 * j_step < 1, a j_q outside 0 .. M - 1, a negative count or offset, or a NaN or infinity in a series a job
 * reads: PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is launched or written.
 * Device work is queued on the context's stream, its memory allocated and freed in stream order; the call
 * returns when the sums are in place. */
typedef struct pw_dft_job {
    int64_t a_first, n;                /* series a = series[a_first .. +n), n <= 2^31 */
    int64_t period;                    /* M: frequencies are j / M cycles per sample, 2 <= M <= 2^31 */
    int64_t j_first, j_step, n_freq;   /* j_q = j_first + q * j_step, every 0 <= j_q < M, j_step >= 1 */
    int64_t out_first;                 /* into re[] and im[] */
} pw_dft_job;
int pw_dft_sums(pw_context *ctx, const pw_dft_job *jobs, int64_t n_jobs, const double *series, double *re,
                double *im);
/* ---- gating statistics: how often and for how long a series stays above or below a threshold -------------
 * What fraction of the time a cage admits a guest of diameter d, how often it opens and how long an opening or
 * a closure lasts, for many d at once.  The reference has no counterpart.  Job k has a series
 * a = series[a_first .. +n) and n_thr thresholds d_q = thresholds[d_first + q]; for each of them every entry
 * has a state -- OPEN a[t] >= d, CLOSED a[t] < d, GAP a[t] a NaN (recognised on the bits) -- and the series is
 * cut into maximal runs of equal state; a run's neighbour is a run of the opposite state, a gap run or an end
 * of the series.  Row r = out_first + q of counts holds, at counts[r * PW_GATE_FIELDS + f]:
 *     f = 0, 1    n_open, n_closed                entries in each state
 *     f = 2, 3    open_runs, closed_runs          maximal runs of each state, whatever bounds them
 *     f = 4, 5    longest_open, longest_closed    length of the longest such run (0 if none)
 *     f = 6       openings                        open runs whose LEFT neighbour is a closed run
 *     f = 7       closings                        closed runs whose left neighbour is an open run
 *     f = 8, 9    complete_open_runs, complete_closed_runs      runs bounded by the opposite state on BOTH
 *                 sides, so their true length is known; a run touching a gap or an end is censored
 *     f = 10, 11  complete_open_frames, complete_closed_frames  summed lengths of the complete runs
 * With n_bins = B > 0, hist[(r * 2 + s) * B + min(len, B) - 1] counts the COMPLETE runs of length len, s = 0
 * open, s = 1 closed; the last bin takes every length >= B.  With B == 0 hist may be NULL and is not touched.
 * Every output is an integer, so the result is this definition itself on every device, launch geometry and
 * run and on a device == -1 context (host threads), whatever else shares the call; the workspace of one call
 * stays within 64 MiB whatever the number of thresholds -- they go through 256 at a time at the least, at
 * 4 bytes per threshold and 512 entries, so a series of more than 3.3e7 entries takes n / 512 KiB instead, 4 GiB
 * at n = 2^31 -- and the result does not depend on how they were cut for that (pywindow_amd/csrc/pw_gate.hpp).
 * All pointers are host memory.  Any mix of job sizes in one call; a job with n == 0 or n_thr == 0 writes
 * nothing; jobs may share entries of `series` and `thresholds` but not rows of `counts` / `hist`; thresholds
 * in any order, repeats allowed.  An infinity in a series a job reads, a NaN or an infinity among the
 * thresholds it reads, n > 2^31, a negative count, offset or n_bins, or hist == NULL with n_bins > 0:
 * PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is launched or written.  Device work
 * is queued on the context's stream, its memory allocated and freed in stream order; the call returns when the
 * counts are in place. */
#define PW_GATE_FIELDS 12
typedef struct pw_gate_job {
    int64_t a_first, n;                /* series a = series[a_first .. +n), n <= 2^31; a NaN entry is a GAP */
    int64_t d_first, n_thr;            /* thresholds d_q = thresholds[d_first + q], q < n_thr */
    int64_t out_first;                 /* row out_first + q of counts[] (and of hist[]) belongs to threshold q */
} pw_gate_job;
int pw_gate_counts(pw_context *ctx, const pw_gate_job *jobs, int64_t n_jobs, const double *series,
                   const double *thresholds, int64_t n_bins, int64_t *counts, int64_t *hist);
/* ---- trajectory kinetics: lagged state-transition counts of a series ---------------------------------------
 * What the rates between the states of a cage are and whether the process is Markovian at the frame spacing:
 * C_k[i][j] = #{t : s[t] = i, s[t + k] = j} for many lags k, from which the transition matrices, populations,
 * implied timescales and the Chapman-Kolmogorov test follow.  The reference has no counterpart.  Job k has a
 * series a = series[a_first .. +n), n_edges strictly increasing edges e = edges[e_first .. +n_edges) and n_lags
 * lags k_q = lag_first + q * lag_step.  The state of a non-NaN entry is the number of the job's edges with
 * e <= a[t] (np.searchsorted(edges, a, side="right"): an entry equal to an edge is in the upper state, and so
 * is -0.0 at an edge 0.0); a NaN entry -- recognised on the bits -- is a GAP.  Row r = out_first + q holds
 *     counts[r * n_states * n_states + i * n_states + j] = the number of t with 0 <= t, t + k_q < n, neither
 *     entry a gap, s[t] = i and s[t + k_q] = j;
 * a pair with a gap at either end is counted nowhere.  Lag 0 gives the populations on the diagonal; a lag >= n
 * gives a row of zeros, which is written; states that a job's edges cannot reach (i, j > n_edges) are zeros of
 * the row, also written.  1 <= n_states <= PW_TRANS_MAX_STATES holds for the whole call.
 * Every output is an integer, so the result is this definition itself on every device, launch geometry and
 * run and on a device == -1 context (host threads), whatever else shares the call.  The device classifies every
 * entry once into one bit mask a state, n_states rounded up to 2, 4, 8 or 16 times n / 8 bytes a job; jobs share
 * a launch while their masks stay within 64 MiB, and a job whose masks alone are more goes alone -- at 16 states
 * a series of more than 3.3e7 entries, 2 n bytes, 4 GiB at n = 2^31 -- and the result does not depend on how the
 * jobs were cut for that (pywindow_amd/csrc/pw_trans.hpp).
 * All pointers are host memory.  Any mix of jobs in one call; a job with n == 0 or n_lags == 0 writes nothing;
 * jobs may share entries of `series` and `edges` but not rows of `counts`, and rows no job owns are never
 * touched.  An infinity in a series a job reads, a NaN, an infinity or a pair that does not increase among the
 * edges it reads, n_edges >= n_states, n > 2^31, a negative field, lag_step < 1, a largest lag of 2^62 or more,
 * or n_states outside 1 .. 16: PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is
 * launched or written.  Device work is queued on the context's stream, its memory allocated and freed in stream
 * order; the call returns when the counts are in place. */
#define PW_TRANS_MAX_STATES 16
typedef struct pw_trans_job {
    int64_t a_first, n;                /* series a = series[a_first .. +n), n <= 2^31; a NaN entry is a GAP */
    int64_t e_first, n_edges;          /* edges e = edges[e_first .. +n_edges), strictly increasing, n_edges < n_states */
    int64_t lag_first, lag_step, n_lags;   /* lags k_q = lag_first + q * lag_step, lag_first >= 0, lag_step >= 1 */
    int64_t out_first;                 /* row out_first + q of counts[] belongs to lag k_q */
} pw_trans_job;
int pw_trans_counts(pw_context *ctx, const pw_trans_job *jobs, int64_t n_jobs, const double *series,
                    const double *edges, int64_t n_states, int64_t *counts);
/* ---- superposition: the rotation that brings one set of points onto another, and their RMSD ------------------
 * The least-squares fit of a frame onto a reference (Horn's quaternion method), the first step of every question
 * about one particular window of a tumbling cage, and the pairwise RMSD behind conformational clustering.  The
 * reference has no counterpart.  Job k has n mobile points x = xyz[mobile_first .. +n) and n target points
 * y = xyz[target_first .. +n) (rows of three doubles; the same rows, or rows other jobs use, are fine) and the
 * weights w = weights[weight_first .. +n), or 1.0 for every point when weight_first == -1.  Row `out` of the
 * result holds the proper rotation R (det +1, also for a mirror-image target and for n = 1, 2, collinear or
 * planar sets, where it is *a* minimiser), the weighted centroids, so that R (x - centre_mobile) + centre_target
 * lies on y, rmsd = sqrt(sum w |R (x - cx) - (y - cy)|^2 / sum w) taken as a direct sum of residuals, the two
 * largest eigenvalues of Horn's 4 x 4 matrix (their gap says how well R is determined) and the Jacobi sweeps.
 * The result is DEFINED: 64 strided accumulators a sum folded pairwise, a cyclic Jacobi with a written sweep rule
 * (pywindow_amd/csrc/pw_superpose.hpp), the same bits on every device, launch geometry and run and on a
 * device == -1 context (host threads), whatever else shares the call and however the jobs are cut into launches
 * to keep the workspace within 16 MiB (28 doubles a job).
 * All pointers are host memory; n_points is the number of rows of xyz and of entries of weights (weights may be
 * null when no job has any).  Jobs may not share rows of `out`; rows no job owns are never touched.  n < 1, a
 * range outside the arrays, a coordinate a job reads that is not finite, a weight it reads that is negative or not
 * finite, or weights that sum to 0: PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is
 * launched or written.  Device work is queued on the context's stream, its memory allocated and freed in stream
 * order; the call returns when the rows are in place. */
typedef struct pw_superpose_job {
    int64_t mobile_first, target_first; /* first rows of the two point sets in xyz */
    int64_t weight_first;               /* first weight, or -1: every weight is 1.0 */
    int64_t n;                          /* points, >= 1 */
    int64_t out;                        /* the job's row of the result */
} pw_superpose_job;
typedef struct pw_superpose_out {
    double rotation[3][3];
    double centre_mobile[3], centre_target[3];
    double rmsd;
    double lambda[2];                   /* the two largest eigenvalues of Horn's matrix, descending */
    int32_t sweeps;
    int32_t reserved;                   /* padding to a multiple of 8 bytes; written as 0 */
} pw_superpose_out;
int pw_superpose(pw_context *ctx, const pw_superpose_job *jobs, int64_t n_jobs, const double *xyz,
                 const double *weights, int64_t n_points, pw_superpose_out *out);
/* ---- conformational clustering of frames: the gromos method over a distance matrix ----------------------------
 * Which conformations a cage visits, which frame stands for each and which conformation every frame is in: the
 * clustering of Daura et al. (1999), GROMACS's `gromos`, over a matrix of pairwise distances such as the RMSD
 * matrix of pw_superpose.  The reference has no counterpart.  Job k has the n x n row-major matrix
 * d = dist[d_first .. + n * n) and a cutoff.  ONLY THE STRICT UPPER TRIANGLE IS READ: the diagonal and the lower
 * triangle may hold anything, a NaN included.  Frames i != j are neighbours iff d[min(i,j)][max(i,j)] <= cutoff;
 * every frame is a neighbour of itself; all frames start active.  While any frame is active:
 *     1. for every active i, count the active neighbours of i, itself included;
 *     2. the centre c is the active frame with the largest count, the SMALLEST INDEX among equal counts;
 *     3. cluster k (0, 1, ... in the order found) is c and its active neighbours: labels[out_first + j] = k for
 *        each of them, centres[out_first + k] = c, sizes[out_first + k] = the count;
 *     4. the members of cluster k become inactive.
 * So sizes do not increase with k, every frame has exactly one label, and n_clusters[k'] of job k' is the number
 * of clusters.  All n entries of centres and sizes are written: past the number of clusters they are -1 and 0.
 * Every output is an integer, so the result is this definition itself on every device, launch geometry and run
 * and on a device == -1 context (host threads), whatever else shares the call.  The device thresholds the matrix
 * once into a bit matrix of n^2 / 8 bytes a job (pywindow_amd/csrc/pw_cluster.hpp); the matrix goes to the device
 * in slabs of whole rows of at most 64 MiB, so it is never there as a whole; jobs share the launches of their
 * rounds while their bit matrices stay within 256 MiB; a round (two launches) finds one cluster of every such
 * job, so a job costs as many rounds as it has clusters and one more; and the result depends on none of that.
 * All pointers are host memory; n_dist is the number of entries of dist.  Any mix of jobs in one call; jobs may
 * share a matrix -- many cutoffs over one matrix, which is then thresholded for each from one upload -- but not
 * entries of labels, centres and sizes; entries no job owns are never touched.  A job with n == 0 writes only
 * its n_clusters = 0.  A NaN in the strict upper triangle of a job's matrix, a NaN cutoff, a negative field,
 * n > PW_CLUSTER_MAX_N or a matrix that reaches outside dist: PW_E_BAD_ARG (pw_last_error names the job and the
 * reason), and nothing is launched or written.  Infinities are legal, in the matrix (never neighbours unless the
 * cutoff is +inf) and as the cutoff (-inf: every frame a cluster of its own).  Device work is queued on the
 * context's stream, its memory allocated and freed in stream order; the call returns when the results are in
 * place. */
#define PW_CLUSTER_MAX_N 32768
typedef struct pw_cluster_job {
    int64_t d_first, n;     /* matrix = dist[d_first .. + n*n), row-major; 0 <= n <= PW_CLUSTER_MAX_N */
    double  cutoff;         /* neighbours: d <= cutoff; any non-NaN value, -inf .. +inf */
    int64_t out_first;      /* labels / centres / sizes [out_first .. +n), n_clusters[its job index] */
} pw_cluster_job;
int pw_cluster_gromos(pw_context *ctx, const pw_cluster_job *jobs, int64_t n_jobs, const double *dist,
                      int64_t n_dist, int32_t *labels, int32_t *centres, int32_t *sizes, int64_t *n_clusters);
/* ---- essential dynamics: column mean and scatter matrix of superposed frames, and projections on modes ---------
 * Which collective motion of the atoms lies behind a trajectory: principal component analysis of the superposed
 * coordinates (Amadei et al. 1993; GROMACS's covar and anaeig).  The reference has no counterpart.  Job k has the
 * row-major matrix X = data[x_first .. + T * D) of T rows and D columns and, when transform_first >= 0, the T rows
 * transforms[transform_first .. + T) of pw_superpose, of which only rotation, centre_mobile and centre_target are
 * read: then D is a multiple of 3, row t is D / 3 points, and each point is taken as
 * y = R_t (x - centre_mobile_t) + centre_target_t, applied as the rows are loaded -- the aligned coordinates never
 * exist anywhere.  Without transforms y = x.
 * pw_covariance writes mean[mean_first .. + D), mean_a = (sum_t y_ta) / T, and, unless s_first == -1 (the mean
 * only), the scatter matrix S = scatter[s_first .. + D * D), row-major, BOTH triangles,
 * S[a][b] = sum_t (y_ta - mean_a)(y_tb - mean_b).  Nothing is divided by T - 1: that is the caller's one IEEE
 * division.  pw_project reads mean[mean_first .. + D) and the k vectors V = vectors[v_first .. + k * D), row-major,
 * and writes P = proj[p_first .. + T * k), P[t][j] = sum_a (y_ta - mean_a) V[j][a].
 * The result is DEFINED (pywindow_amd/csrc/pw_cov.hpp): the transform is three subtractions, one product and two
 * fma a row of R, and one addition; the rows are cut into chunks of PW_COV_CHUNK; a column's chunk sums are
 * sequential in t and are added in chunk order; an entry of S is the sequential fma(z_a, z_b, acc) over a chunk's
 * rows, z = y - mean, the chunk partials added in chunk order, so S is symmetric to the bit and T = 1 gives +0
 * everywhere; an entry of P is taken by 64 accumulators striding over the columns, folded pairwise as in
 * pw_superpose.  No floating-point atomics and no MFMA.  The same bits on every device, launch geometry and run
 * and on a device == -1 context (host threads), whatever else shares the call and however a job's tiles and
 * chunks are cut into launches to keep the workspace within 256 MiB.  There is no capacity in T, nor in D up to
 * PW_COV_MAX_D.
 * All pointers are host memory; n_data, n_transforms, n_mean, n_scatter, n_vectors and n_proj are the entries
 * (rows, for transforms) of the arrays; transforms may be null when no job has any, scatter when every job has
 * s_first == -1.  Jobs may share inputs but not entries of the outputs; entries no job owns are never touched.
 * T < 1, D < 1, D > PW_COV_MAX_D, D % 3 != 0 with transforms, k < 1, a range outside data, the transforms or the
 * outputs, a value a job reads that is not finite, or jobs that share output entries: PW_E_BAD_ARG (pw_last_error
 * names the job and the reason), and nothing is launched or written.  Device work is queued on the context's
 * stream, its memory allocated and freed in stream order; the call returns when the results are in place. */
#define PW_COV_CHUNK 256
#define PW_COV_MAX_D 3072
typedef struct pw_cov_job {
    int64_t x_first;          /* X = data[x_first .. + T * D), row-major */
    int64_t T, D;             /* rows >= 1, columns 1 .. PW_COV_MAX_D */
    int64_t transform_first;  /* first of the T rows of transforms, or -1: none */
    int64_t mean_first;       /* mean[mean_first .. + D) is written */
    int64_t s_first;          /* scatter[s_first .. + D * D) is written, or -1: the mean only */
} pw_cov_job;
int pw_covariance(pw_context *ctx, const pw_cov_job *jobs, int64_t n_jobs, const double *data, int64_t n_data,
                  const pw_superpose_out *transforms, int64_t n_transforms, double *mean, int64_t n_mean,
                  double *scatter, int64_t n_scatter);
typedef struct pw_project_job {
    int64_t x_first;          /* X = data[x_first .. + T * D), row-major */
    int64_t T, D;
    int64_t transform_first;  /* first of the T rows of transforms, or -1: none */
    int64_t mean_first;       /* mean[mean_first .. + D) is READ */
    int64_t v_first, k;       /* V = vectors[v_first .. + k * D), k >= 1 */
    int64_t p_first;          /* proj[p_first .. + T * k) is written */
} pw_project_job;
int pw_project(pw_context *ctx, const pw_project_job *jobs, int64_t n_jobs, const double *data, int64_t n_data,
               const pw_superpose_out *transforms, int64_t n_transforms, const double *mean, int64_t n_mean,
               const double *vectors, int64_t n_vectors, double *proj, int64_t n_proj);
/* ---- the cavity of a cage: a voxel flood fill from the pore centre, closed at the windows ---------------------
 * How much room is inside a cage, what shape it has and how it fluctuates: pore_volume is the volume of the largest
 * inscribed sphere, a lower bound on the cavity; this is the region a probe's CENTRE can reach from a seed without
 * crossing an atom or a plane laid through a window.  The reference has no counterpart.  Job k has
 *     atoms   n >= 0 atoms xyz[atom_first .. +n) (rows of three doubles) with radii[radius_first .. +n), and a
 *             probe radius probe >= 0;
 *     a grid  of nx x ny x nz voxels, each 1 .. PW_CAVITY_MAX_G, with an origin o and a spacing h > 0: voxel
 *             (i, j, l) has the centre x = o_x + (double)i * h, likewise y and z (one product, one addition, no fma);
 *     planes  m >= 0 rows (a, b, c, d) planes[plane_first .. +m);
 *     a seed  voxel (seed[0], seed[1], seed[2]) inside the grid.
 * A voxel is FREE iff for every atom, with dx = x - X and so on,
 *     (dx*dx + dy*dy) + dz*dz >= (radius + probe) * (radius + probe)           (equality is free),
 * and OPEN iff it is free and ((a*x + b*y) + c*z) <= d holds for every plane.  The CAVITY is the 6-connected
 * component of open voxels that contains the seed voxel; it is empty, and PW_CAV_SEED_CLOSED is set, if the seed
 * voxel is not open.  All floating point is FP64 without contraction in exactly the association written.
 * Row `out` of the result holds integers only: the voxels of the cavity (n_voxels) and of the open set (n_open);
 * the cavity voxels with at least one of the six neighbours not in the cavity, a neighbour outside the grid counting
 * as not in it (n_surface); the cavity voxels on a face of the grid (n_face: 0 means that the cavity is closed inside
 * the box); the sums of i, j, l over the cavity (first) and of ii, jj, ll, ij, il, jl (second); the bounding box
 * i_min, i_max, j_min, j_max, l_min, l_max, all -1 when the cavity is empty; and the flags.  Volume
 * (n_voxels * h^3), centroid (o + h * first / n_voxels) and gyration tensor are the caller's few IEEE operations
 * on these integers.  When mask_first >= 0 the cavity itself is written to mask[mask_first .. + ny * nz): one word
 * a row (j, l) of the grid at index l * ny + j, bit i set iff voxel (i, j, l) is in the cavity.
 * Every output is an integer, so the result is this definition itself on every device, launch geometry and run
 * and on a device == -1 context (host threads), whatever else shares the call and however the jobs are cut into
 * launches.  A row of the grid may skip an atom when dy*dy + dz*dz >= (radius + probe)^2, which is exact (rounding
 * is monotone: pywindow_amd/csrc/pw_cavity.hpp); nothing else is culled, and there is no capacity in n or m.
 * All pointers are host memory; n_points, n_radii, n_planes, n_out and n_mask are the rows of xyz, the entries of
 * radii, the rows of planes, the rows of out and the words of mask (arrays no job uses may be null).  Jobs may share
 * atoms, radii and planes but not rows of out or words of mask; entries no job owns are never touched.  A value a
 * job reads that is not finite, h <= 0, a negative radius or probe, a dimension outside 1 .. PW_CAVITY_MAX_G, a
 * seed outside the grid, a range outside an array or jobs that share outputs: PW_E_BAD_ARG (pw_last_error names
 * the job and the reason), and nothing is launched or written.  Device work is queued on the context's stream,
 * its memory allocated and freed in stream order; the call returns when the results are in place. */
#define PW_CAVITY_MAX_G 64
#define PW_CAV_SEED_CLOSED 1     /* the seed voxel is not open: the cavity is empty */
typedef struct pw_cavity_job {
    int64_t atom_first, n;      /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t radius_first;       /* their radii = radii[radius_first .. +n) */
    int64_t plane_first, m;     /* planes = planes[plane_first .. +m), rows (a, b, c, d), m >= 0 */
    int64_t mask_first;         /* mask[mask_first .. + ny*nz) is written, or -1: no mask */
    int64_t out;                /* the job's row of the result */
    double  origin[3];          /* the centre of voxel (0, 0, 0) */
    double  spacing;            /* h > 0 */
    double  probe;              /* >= 0 */
    int32_t nx, ny, nz;         /* 1 .. PW_CAVITY_MAX_G */
    int32_t seed[3];            /* the seed voxel (i, j, l) */
} pw_cavity_job;
typedef struct pw_cavity_out {
    int64_t n_voxels, n_open, n_surface, n_face;
    int64_t first[3];           /* sums of i, j, l over the cavity */
    int64_t second[6];          /* sums of ii, jj, ll, ij, il, jl */
    int32_t box[6];             /* i_min, i_max, j_min, j_max, l_min, l_max; -1 when the cavity is empty */
    int32_t flags;              /* PW_CAV_* */
    int32_t reserved;           /* padding to a multiple of 8 bytes; written as 0 */
} pw_cavity_out;
int pw_cavity(pw_context *ctx, const pw_cavity_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
              const double *radii, int64_t n_radii, const double *planes, int64_t n_planes, pw_cavity_out *out,
              int64_t n_out, uint64_t *mask, int64_t n_mask);
/* ---- the accessible surface of a cage, and which side of it faces the cavity ----------------------------------
 * The solvent-accessible surface for a probe of a given radius by test points (Shrake and Rupley, 1973), every point
 * attributed to the cavity or to the outside with the bit mask of pw_cavity.  The reference has no counterpart.
 * The call has P = n_directions unit directions u_k = directions[3k .. 3k + 3), 1 <= P <= PW_SASA_MAX_POINTS, shared
 * by its jobs.  Job k has
 *     atoms   n >= 0 atoms xyz[atom_first .. +n) (rows of three doubles) with radii[radius_first .. +n), and a
 *             probe radius probe >= 0;
 *     a grid  when word_first >= 0: nx x ny x nz voxels, each 1 .. PW_CAVITY_MAX_G, with an origin o and a spacing
 *             h > 0, and the ny * nz words words[word_first ..) in the layout of pw_cavity's mask -- row (j, l) at
 *             index l * ny + j, bit i voxel i.  word_first == -1: no grid; origin, spacing and nx, ny, nz are not read.
 * Atom i has the reach R_i = radius_i + probe and the test points p = X_i + R_i * u_k, component by component (one
 * product, one addition, no fma).  A point is EXPOSED iff for every atom j != i (excluded by index, not by position)
 *     (dx*dx + dy*dy) + dz*dz >= R_j * R_j,   dx = p_x - X_j,x, ...                (equality is exposed),
 * so a second atom at the same position is another atom -- with a larger reach it buries every point --, and an atom
 * of radius 0 with probe 0 buries nothing.  An exposed point is INSIDE iff the job has a grid and at least one of the up to eight
 * voxels at the corners of the grid cell that holds p is set in the words: along x, i0 is the largest i in [0, nx)
 * with o_x + (double)i * h <= p_x, or -1; the corners are i0 and i0 + 1, those outside [0, nx) dropped; y and z
 * likewise.  Nothing is divided; bits at i >= nx are ignored; a point with no corner in the grid is not inside.
 * All floating point is FP64 without contraction in exactly the association written.
 * Written: exposed[count_first + i] and inside[count_first + i], the numbers of exposed and of inside points of atom
 * i, and row `out` of the result with their sums over the job and the flags (PW_SASA_GRID: the job had a grid).
 * Areas (4 pi R_i^2 exposed_i / P) are the caller's few IEEE operations on these integers.  Every output is an
 * integer, so the result is this definition itself on every device, launch geometry and run and on a device == -1
 * context (host threads).  An atom j is skipped for atom i only when the centres are further apart than the sum of
 * the reaches by a margin that covers every rounding and the tolerance on |u| (pywindow_amd/csrc/pw_sasa.hpp has the
 * rule and its proof; it is not applied when the job's largest magnitude is outside 2^-400 .. 2^400); there is no
 * capacity in n.
 * All pointers are host memory; n_points, n_radii, n_words, n_counts and n_out are the rows of xyz, the entries of
 * radii, of words, of exposed and of inside (each n_counts) and the rows of out (arrays no job uses may be null).
 * Jobs may share atoms, radii and words but not rows of out or entries of exposed / inside; entries no job owns are
 * never touched.  A value a job reads that is not finite, a negative radius or probe, h <= 0, a dimension outside
 * 1 .. PW_CAVITY_MAX_G, a range outside an array, jobs that share outputs: PW_E_BAD_ARG (pw_last_error names the
 * job and the reason), and nothing is launched or written.  The directions are read by the jobs that have atoms: the
 * first of them is the one named when P is outside its range, a direction is not finite or
 * |((ux*ux + uy*uy) + uz*uz) - 1| > 1e-9 (the message names the direction too).  Device work is queued on the
 * context's stream, its memory allocated and freed in stream order; the call returns when the results are in place. */
#define PW_SASA_MAX_POINTS 4096
#define PW_SASA_GRID 1            /* flags: the job had a grid */
typedef struct pw_sasa_job {
    int64_t atom_first, n;      /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t radius_first;       /* their radii = radii[radius_first .. +n) */
    int64_t count_first;        /* exposed[count_first .. +n) and inside[count_first .. +n) are written */
    int64_t word_first;         /* the grid's words = words[word_first .. + ny*nz), or -1: no grid */
    int64_t out;                /* the job's row of the result */
    double  origin[3];          /* the centre of voxel (0, 0, 0) */
    double  spacing;            /* h > 0 */
    double  probe;              /* >= 0 */
    int32_t nx, ny, nz;         /* 1 .. PW_CAVITY_MAX_G */
    int32_t reserved;           /* padding to a multiple of 8 bytes; not read */
} pw_sasa_job;
typedef struct pw_sasa_out {
    int64_t exposed, inside;    /* sums of the per-atom counts */
    int32_t flags;              /* PW_SASA_* */
    int32_t reserved;           /* padding to a multiple of 8 bytes; written as 0 */
} pw_sasa_out;
int pw_sasa(pw_context *ctx, const pw_sasa_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
            const double *radii, int64_t n_radii, const double *directions, int64_t n_directions,
            const uint64_t *words, int64_t n_words, int32_t *exposed, int32_t *inside, int64_t n_counts,
            pw_sasa_out *out, int64_t n_out);
/* ---- pore sizes: the probe-swept cavity for a ladder of probes ---------------------------------------------------
 * The room a guest of radius p can actually fill (the probe-occupiable volume: the reach of the probe's centre
 * dilated by the probe sphere; Ongari et al., Langmuir 2017) and the geometric pore size distribution (for every
 * point of the void the largest sphere that contains it, fits between the atoms and can be brought there from the
 * pore centre; Gelb and Gubbins 1999), whose cumulative form at radius p is that volume.  The reference has no
 * counterpart.  Job k has the atoms, radii, planes, grid (nx, ny, nz in 1 .. PW_CAVITY_MAX_G, origin o, spacing
 * h > 0) and seed voxel of a pw_cavity job, and L = n_levels probe radii probes[probe_first .. +L),
 * 1 <= L <= PW_PORES_MAX_LEVELS, each finite and >= 0, strictly ascending: p_0 < p_1 < ... < p_{L-1}.  Per level l:
 *     reach_l   the cavity of pw_cavity for the probe p_l -- the same voxel centres, (radius + p_l)^2, free and open
 *               tests in the same association, the 6-connected fill from the seed voxel; it is empty, and
 *               PW_CAV_SEED_CLOSED is in the level's flags, if the seed voxel is not open at that level;
 *     K_l       the largest integer k in [0, PW_PORES_MAX_K2] with (double)k * (h * h) <= p_l * p_l, each product
 *               rounded once (the left side is monotone in k: a bisection, nothing is divided);
 *     swept_l   the voxels v of the grid for which some c in reach_l has
 *               (v_i-c_i)^2 + (v_j-c_j)^2 + (v_l-c_l)^2 <= K_l in integers.  Voxels outside the grid do not exist:
 *               nothing wraps and nothing reaches bits >= nx.
 * domain = reach_0, and for v in domain cover(v) is the largest l with v in swept_l, or none.  Integers only are
 * written.  Row level_first + l of levels: n_reach and n_face (pw_cavity's n_voxels and n_face for p_l),
 * n_swept = |swept_l & domain|, n_largest = #{v in domain : cover(v) = l}, k2 = K_l and the flags.  Row `out` of
 * out: n_domain, n_none = #{v in domain without a cover} and n_levels, with n_domain = n_none + sum_l n_largest_l.
 * (A ball holds its centre whatever K is, so swept_0 holds reach_0: n_swept_0 = n_domain and n_none = 0 under this
 * definition.)  When mask_first >= 0 the words of swept_l & domain go to mask[mask_first + l * ny * nz ..), level
 * after level, each in the layout of pw_cavity's mask.  Volumes are the caller's count * h^3.  The resolution in p
 * is the grid's: a probe below h has K = 0 and sweeps nothing beyond its centres, and the raw n_swept need not be
 * monotone in p on a grid -- the reverse cumulative sum of n_largest is.
 * Every output is an integer and the sweep has no floating point (pywindow_amd/csrc/pw_pores.hpp), so the result is
 * this definition itself on every device, launch geometry and run and on a device == -1 context (host threads).
 * All pointers are host memory; n_points, n_radii, n_planes, n_probes, n_levels, n_out and n_mask are the rows of
 * xyz, the entries of radii, the rows of planes, the entries of probes, the rows of levels and of out and the words of
 * mask (arrays no job uses may be null).  Jobs may share atoms, radii, planes and probes but not rows of out, rows
 * of levels or words of mask; entries no job owns are never touched.  What pw_cavity refuses, L outside its range,
 * a probe that is not finite or negative, probes not strictly ascending, a range outside an array or jobs that
 * share outputs: PW_E_BAD_ARG (pw_last_error names the job and the reason), and nothing is launched or written.
 * Device work is queued on the context's stream, its memory allocated and freed in stream order; the call returns
 * when the results are in place. */
#define PW_PORES_MAX_LEVELS 64
#define PW_PORES_MAX_K2 11907     /* 3 * 63 * 63: the squared distance of opposite corners of a 64^3 grid */
typedef struct pw_pores_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t radius_first;           /* their radii = radii[radius_first .. +n) */
    int64_t plane_first, m;         /* planes = planes[plane_first .. +m), rows (a, b, c, d), m >= 0 */
    int64_t probe_first, n_levels;  /* the ladder = probes[probe_first .. +n_levels) */
    int64_t level_first;            /* levels[level_first .. +n_levels) is written */
    int64_t mask_first;             /* mask[mask_first .. + n_levels*ny*nz) is written, or -1: no mask */
    int64_t out;                    /* the job's row of out */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  spacing;                /* h > 0 */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t seed[3];                /* the seed voxel (i, j, l) */
} pw_pores_job;
typedef struct pw_pores_level {
    int64_t n_reach, n_face;        /* pw_cavity's n_voxels and n_face for this probe */
    int64_t n_swept;                /* |swept_l & domain| */
    int64_t n_largest;              /* #{v in domain : cover(v) = l} */
    int32_t k2;                     /* K_l */
    int32_t flags;                  /* PW_CAV_SEED_CLOSED */
} pw_pores_level;
typedef struct pw_pores_out {
    int64_t n_domain, n_none, n_levels;
} pw_pores_out;
int pw_pore_sizes(pw_context *ctx, const pw_pores_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
                  const double *radii, int64_t n_radii, const double *planes, int64_t n_planes, const double *probes,
                  int64_t n_probes, pw_pores_level *levels, int64_t n_levels, pw_pores_out *out, int64_t n_out,
                  uint64_t *mask, int64_t n_mask);
/* ---- guest affinity: the Lennard-Jones energy map of a cavity and its Boltzmann sums -----------------------------
 * How strongly a cage holds a one-site guest: the Boltzmann-weighted volume of the cavity (the helium void volume,
 * the Henry coefficient), the mean and the minimum binding energy and an energy histogram, at up to
 * PW_AFF_MAX_LEVELS temperatures in one pass.  The reference has no counterpart.  Job k has
 *     atoms   n >= 0 atoms xyz[atom_first .. +n) (rows of three doubles) with rows (A, B) coef[coef_first .. +n),
 *             finite, 0 <= A, B <= 1e100.  A = 4 eps sigma^12 and B = 4 eps sigma^6 are the caller's (units included);
 *     a grid  nx x ny x nz voxels, each 1 .. PW_CAVITY_MAX_G, origin o and spacing h > 0 exactly as pw_cavity: voxel
 *             (i, j, l) has the centre x = o_x + (double)i * h, likewise y and z;
 *     region  the ny * nz words words[word_first ..) in the layout of pw_cavity's mask -- row (j, l) at l * ny + j, bit
 *             i voxel i, bits at i >= nx ignored; word_first == -1: every voxel of the grid;
 *     core2 >= 1e-6 and cutoff2 (0.0: no cutoff, otherwise > core2), both finite;
 *     L = n_betas inverse temperatures betas[beta_first .. +L), 1 <= L <= PW_AFF_MAX_LEVELS, finite and >= 0;
 *     E = n_edges histogram edges edges[edge_first .. +E), 0 <= E <= PW_AFF_MAX_EDGES, finite, strictly ascending.
 * ORDER.  The voxels of the region are ranked by (l, j, i) ascending; V is their number.
 * ENERGY.  Per voxel, the atoms in index order, dx = x - X and so on, r2 = (dx*dx + dy*dy) + dz*dz.  The voxel is
 * BLOCKED iff some atom has r2 <= core2.  An atom COUNTS iff cutoff2 == 0.0 or r2 <= cutoff2; an atom that does not
 * count is skipped, not added as zero.  For a counting atom q = 1.0 / r2 (correctly rounded), s = (q*q)*q,
 * u = s * (A*s - B), U = U + u, from +0.0.  The bounds keep U of a voxel that is not blocked finite.
 * WEIGHT.  Per beta and voxel that is not blocked: x = -(beta * U); if x > 700.0 then x = 700.0 and PW_AFF_CLAMPED
 * is set in the job's flags; w = pw_exp(x) (pywindow_amd/csrc/pw_math.hpp); the terms are z = w and e = w * U.
 * SUMS.  Chunk c holds the ranks 64c .. 64c + 63; a slot whose rank is >= V or whose voxel is blocked holds +0.0.
 * Within a chunk, for k = 1, 2, 4, 8, 16, 32 in turn, slot[t] = slot[t] + slot[t + k] for every t that is a multiple
 * of 2k; the chunk's sum is slot[0].  The total starts at +0.0 and takes the chunk sums in chunk order.  There are
 * no floating-point atomics.  All floating point is FP64 without contraction in exactly the association written, so
 * the result is the same bytes on every device, launch geometry and run and on a device == -1 context (host
 * threads), whatever else shares the call and however the jobs are cut into launches.
 * Written: row `out` (n_voxels = V, n_blocked, u_min -- the smallest U of a voxel that is not blocked, ties to the
 * lowest rank; +inf and min_voxel = -1 when there is none --, min_voxel = (i, j, l) and the flags); rows
 * levels[level_first + b] = (Z_b, E_b), the totals of z and e; hist[hist_first + k] = #{v not blocked :
 * U_v < edge_k}, by comparisons; and, when energy_first >= 0, energies[energy_first + rank] = U, +inf where blocked.
 * The Boltzmann volume Z h^3, the mean energy E / Z and everything built on them are the caller's.
 * All pointers are host memory; n_points, n_coef, n_words, n_betas, n_edges, n_energies, n_levels, n_hist and n_out
 * are the rows of xyz and of coef, the entries of words, betas, edges and energies, the rows of levels, the entries of
 * hist and the rows of out (arrays no job uses may be null).  Jobs may share every input but no row of out or of
 * levels and no entry of hist or energies; entries no job owns are never touched.  A value a job reads that is not
 * finite or outside its bounds, a dimension or a count outside its range, a range outside an array or jobs that
 * share outputs: PW_E_BAD_ARG (pw_last_error names the job -- of two that share, the later -- and the reason), and
 * nothing is launched or written.  Device work is queued on the context's stream, its memory allocated and freed in
 * stream order; there is no capacity in n; the call returns when the results are in place. */
#define PW_AFF_MAX_LEVELS 8
#define PW_AFF_MAX_EDGES 16
#define PW_AFF_CLAMPED 1          /* flags: some -(beta * U) was above 700 and was taken as 700 */
typedef struct pw_affinity_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t coef_first;             /* their rows (A, B) = coef[coef_first .. +n) */
    int64_t word_first;             /* the region = words[word_first .. + ny*nz), or -1: every voxel */
    int64_t beta_first, n_betas;    /* betas[beta_first .. +n_betas) */
    int64_t edge_first, n_edges;    /* edges[edge_first .. +n_edges) */
    int64_t level_first;            /* levels[level_first .. +n_betas) is written */
    int64_t hist_first;             /* hist[hist_first .. +n_edges) is written */
    int64_t energy_first;           /* energies[energy_first .. +V) is written, or -1: no energy map */
    int64_t out;                    /* the job's row of out */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  spacing;                /* h > 0 */
    double  core2;                  /* >= 1e-6 */
    double  cutoff2;                /* 0.0: none; otherwise > core2 */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t reserved;               /* padding to a multiple of 8 bytes; not read */
} pw_affinity_job;
typedef struct pw_affinity_level {
    double z, e;                    /* sum of w, sum of w * U */
} pw_affinity_level;
typedef struct pw_affinity_out {
    int64_t n_voxels, n_blocked;
    double  u_min;
    int32_t min_voxel[3];           /* (i, j, l), or -1 */
    int32_t flags;                  /* PW_AFF_* */
} pw_affinity_out;
int pw_affinity(pw_context *ctx, const pw_affinity_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
                const double *coef, int64_t n_coef, const uint64_t *words, int64_t n_words, const double *betas,
                int64_t n_betas, const double *edges, int64_t n_edges, double *energies, int64_t n_energies,
                pw_affinity_level *levels, int64_t n_levels, int64_t *hist, int64_t n_hist, pw_affinity_out *out,
                int64_t n_out);
/* ---- guest passage: the barrier a guest crosses at every window -----------------------------------------------
 * Whether a guest can get in or out through a window, and at what cost: the minimax (bottleneck) level of a scalar
 * field between a seed voxel and the faces of its box, once per window with the other windows' planes shut.  The
 * reference has no counterpart.  Job k has the grid (nx, ny, nz in 1 .. PW_CAVITY_MAX_G, origin o, spacing h > 0, voxel
 * centres x = o_x + (double)i * h), the seed voxel and the m >= 0 planes planes[plane_first .. +m) of a pw_cavity job,
 * and a field U over every voxel of the grid, the voxels ranked by (l, j, i) ascending as in pw_affinity:
 *     field_first == -1   the Lennard-Jones energy of pw_affinity's ENERGY paragraph from the atoms xyz[atom_first ..
 *                         +n), their rows (A, B) coef[coef_first .. +n), core2 and cutoff2 -- the same operations in
 *                         the same order and association --, +inf at a blocked voxel;
 *     field_first >= 0    the caller's field[field_first .. + nx*ny*nz): every value finite or +inf (+inf: blocked);
 *                         atoms, coefficients, core2 and cutoff2 are not read.  Any scalar field will do: the negative
 *                         distance to the nearest atom surface gives the largest hard sphere that passes.
 * R = max(m, 1) rows out[out_first .. +R) are written.  Row k leaves plane k out; with m == 0 the one row has no plane.
 * For row k, held(v) iff ((a*x + b*y) + c*z) <= d for every plane j != k; allowed_t(v) iff U_v is not +inf, held(v) and
 * U_v <= t; F(t) is the 6-connected component of allowed_t that holds the seed voxel, empty if the seed voxel is not
 * allowed; P(t) iff F(t) has a voxel on a face of the grid (pw_cavity's n_face notion).  P is monotone in t and
 * changes only at voxel values.  The row holds u_seed = U of the seed voxel and
 *     PW_PAS_SEED_CLOSED  the seed voxel is blocked or not held: barrier = well = +inf, every voxel -1, every count 0;
 *     PW_PAS_NO_EXIT      P is false at the largest finite U: barrier = +inf, saddle = -1, and the rest as below at
 *                         t = +inf (so n_basin = n_fill);
 *     barrier B           the smallest voxel value t with P(t), as the bits of U at the saddle;
 *     n_fill              |F(B)|;
 *     saddle              the voxel (i, j, l) of F(B) with U == B of the lowest rank.  A -0.0 compares equal to +0.0;
 *                         barrier is whichever of the two the saddle holds;
 *     well, well_voxel    the smallest U over F(B), ties to the lowest rank by strict < in rank order;
 *     n_basin             the size of the seed's component of {allowed, U < B} (strict), 0 when U_seed == B.
 * Everything is a comparison of doubles or an integer count, all floating point FP64 without contraction in exactly the
 * association written, so the result is this definition itself on every device, launch geometry and run and on a
 * device == -1 context (host threads), whatever else shares the call and however the jobs are cut into launches.
 * A saddle on a face of the box means that the window is no obstacle of its own: the barrier is then the energy where
 * the path left the box and depends on the box.  The activation energy barrier - well is the caller's.
 * All pointers are host memory; n_points, n_coef, n_planes, n_field and n_out are the rows of xyz, of coef and of
 * planes, the entries of field and the rows of out (arrays no job uses may be null).  Jobs may share every input but no
 * row of out; entries no job owns are never touched.  What pw_cavity and pw_affinity refuse for the same fields, a
 * field value that is -inf or not a number, a range outside an array or jobs that share rows of out: PW_E_BAD_ARG
 * (pw_last_error names the job -- of two that share, the later -- and the reason), and nothing is launched or written.
 * Device work is queued on the context's stream, its memory allocated and freed in stream order; there is no capacity in
 * n or m; the call returns when the results are in place. */
#define PW_PAS_SEED_CLOSED 1      /* flags: the seed voxel is blocked or not held */
#define PW_PAS_NO_EXIT 2          /* flags: no level connects the seed to a face of the grid */
typedef struct pw_passage_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n) (read when field_first == -1); n >= 0 always */
    int64_t coef_first;             /* their rows (A, B) = coef[coef_first .. +n) */
    int64_t plane_first, m;         /* planes = planes[plane_first .. +m), rows (a, b, c, d), m >= 0 */
    int64_t field_first;            /* U = field[field_first .. + nx*ny*nz), or -1: the Lennard-Jones energy */
    int64_t out_first;              /* out[out_first .. + max(m, 1)) is written */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  spacing;                /* h > 0 */
    double  core2;                  /* >= 1e-6 (read when field_first == -1) */
    double  cutoff2;                /* 0.0: none; otherwise > core2 */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t seed[3];                /* the seed voxel (i, j, l) */
} pw_passage_job;
typedef struct pw_passage_out {
    double  barrier, well, u_seed;
    int64_t n_fill, n_basin;
    int32_t saddle[3];              /* (i, j, l), or -1 */
    int32_t well_voxel[3];          /* (i, j, l), or -1 */
    int32_t flags;                  /* PW_PAS_* */
    int32_t reserved;               /* padding to a multiple of 8 bytes; written as 0 */
} pw_passage_out;
int pw_passage(pw_context *ctx, const pw_passage_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
               const double *coef, int64_t n_coef, const double *planes, int64_t n_planes, const double *field,
               int64_t n_field, pw_passage_out *out, int64_t n_out);
/* ---- guest hopping: the free-energy profile of a guest through a window -----------------------------------------
 * How fast a guest hops out: transition-state theory needs the Boltzmann-weighted area of the dividing surface in a
 * window and the Boltzmann-weighted volume of the well behind it, k = sqrt(k_B T / 2 pi m) * A / V_well.  pw_hop gives
 * both, slab by slab along the window's axis.  The reference has no counterpart.  Job k is one (frame, window) in that
 * window's own frame: the caller has rotated atoms and planes so that the window's axis is z.  It has
 *     a grid   nx x ny x nz voxels, each 1 .. PW_CAVITY_MAX_G, origin o and spacing h > 0 exactly as pw_cavity: voxel
 *              (i, j, l) has the centre x = o_x + (double)i * h, likewise y and z, and the rank (l, j, i);
 *     a seed   column (si, sj) = seed[0 .. 2) inside the grid;
 *     planes   m >= 0 planes planes[plane_first .. +m), rows (a, b, c, d), ALL of them held (the caller leaves its own
 *              window's plane out);
 *     a field  U exactly as in pw_passage: field_first == -1 is the Lennard-Jones energy of pw_affinity's ENERGY
 *              paragraph from xyz[atom_first .. +n), coef[coef_first .. +n), core2 and cutoff2, +inf at a blocked voxel;
 *              field_first >= 0 is the caller's field[field_first .. + nx*ny*nz), every value finite or +inf;
 *     cap      a finite double, and L = n_betas inverse temperatures betas[beta_first .. +L), 1 <= L <=
 *              PW_AFF_MAX_LEVELS, finite and >= 0.
 * For every slab l on its own: allowed(i, j) iff U is not +inf, ((a*x + b*y) + c*z) <= d for every plane and U <= cap.
 * C_l is the 4-connected component, in (i, j) only, of allowed that holds (si, sj), empty when that voxel is not
 * allowed.  n = |C_l|; n_face = the voxels of C_l with i == 0, i == nx - 1, j == 0 or j == ny - 1, each counted once;
 * u_min = the smallest U over C_l as the bits its voxel (min_i, min_j) holds, ties (a -0.0 with a +0.0 as well) to the
 * lowest (j, i); +inf and -1, -1 when C_l is empty.  Per beta the sums (Z, E) of pw_affinity's WEIGHT and SUMS
 * paragraphs over the voxels of C_l ranked by (j, i): x = -(beta * U), x > 700.0 taken as 700.0 with PW_HOP_CLAMPED in
 * the job's flags, w = pw_exp(x), the terms z = w and e = w * U, chunks of 64 ranks summed by the same tree and added in
 * order from +0.0 -- with C_l handed to pw_affinity as a one-slab mask (Z, E) are pw_affinity's bytes.
 * Written: slabs[slab_first + l] for l = 0 .. nz - 1; sums[sum_first + l * L + b] = (Z, E); row `out` (the total of n
 * and the flags); and, when word_first >= 0, words[word_first + l * ny + j] = row j of C_l, bit i voxel i -- the layout
 * of pw_cavity's mask.  All floating point is FP64 without contraction in exactly the association written and there are
 * no floating-point atomics, so the result is the same bytes on every device, launch geometry and run and on a
 * device == -1 context (host threads), whatever else shares the call and however the jobs are cut into launches.
 * The area h^2 Z of a slab, the volume h^3 sum Z of a run of slabs and the rate built on them are the caller's.
 * All pointers are host memory; n_points, n_coef, n_planes, n_field, n_betas, n_slabs, n_sums, n_out and n_words are the
 * rows of xyz, of coef and of planes, the entries of field and of betas, the rows of slabs, of sums and of out and the
 * entries of words (arrays no job uses may be null).  Jobs may share every input but no output; entries no job owns are
 * never touched.  What pw_passage refuses for the same fields, a cap that is not finite, a seed column outside the
 * grid, n_betas outside its range, a beta that is negative or not finite, a range outside an array or jobs that share
 * outputs: PW_E_BAD_ARG (pw_last_error names the job -- of two that share, the later -- and the reason), and nothing
 * is launched or written.  Device work is queued on the context's stream, its memory allocated and freed in stream
 * order; there is no capacity in n or m; the call returns when the results are in place. */
#define PW_HOP_CLAMPED 1          /* flags: some -(beta * U) was above 700 and was taken as 700 */
typedef struct pw_hop_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n) (read when field_first == -1); n >= 0 always */
    int64_t coef_first;             /* their rows (A, B) = coef[coef_first .. +n) */
    int64_t plane_first, m;         /* planes = planes[plane_first .. +m), rows (a, b, c, d), m >= 0 */
    int64_t field_first;            /* U = field[field_first .. + nx*ny*nz), or -1: the Lennard-Jones energy */
    int64_t beta_first, n_betas;    /* betas[beta_first .. +n_betas) */
    int64_t slab_first;             /* slabs[slab_first .. +nz) is written */
    int64_t sum_first;              /* sums[sum_first .. + nz*n_betas) is written */
    int64_t word_first;             /* words[word_first .. + ny*nz) is written, or -1: no words */
    int64_t out;                    /* the job's row of out */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  spacing;                /* h > 0 */
    double  core2;                  /* >= 1e-6 (read when field_first == -1) */
    double  cutoff2;                /* 0.0: none; otherwise > core2 */
    double  cap;                    /* finite: a voxel above it is not allowed */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t seed[2];                /* the seed column (si, sj) */
    int32_t reserved;               /* padding to a multiple of 8 bytes; not read */
} pw_hop_job;
typedef struct pw_hop_slab {
    int64_t n, n_face;
    double  u_min;
    int32_t min_i, min_j;           /* or -1, -1 */
} pw_hop_slab;
typedef struct pw_hop_out {
    int64_t n;                      /* the total of the slabs' n */
    int32_t flags;                  /* PW_HOP_* */
    int32_t reserved;               /* padding to a multiple of 8 bytes; written as 0 */
} pw_hop_out;
int pw_hop(pw_context *ctx, const pw_hop_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
           const double *coef, int64_t n_coef, const double *planes, int64_t n_planes, const double *field,
           int64_t n_field, const double *betas, int64_t n_betas, pw_hop_slab *slabs, int64_t n_slabs,
           pw_affinity_level *sums, int64_t n_sums, pw_hop_out *out, int64_t n_out, uint64_t *words, int64_t n_words);
/* ---- rigid linear guests: the orientation-averaged affinity of a cavity ------------------------------------------
 * pw_affinity for a guest that is not a sphere: a rigid linear molecule (N2, CO2, O2 -- sites on one axis, optional
 * point charges) inserted at every voxel of a region in every one of M orientations, the Boltzmann sums averaged over
 * the orientations.  The reference has no counterpart.  Job k has the grid, the region (word_first, or -1: every
 * voxel), core2, cutoff2 and the L = n_betas betas exactly as a pw_affinity job, n >= 0 atoms xyz[atom_first .. +n), and
 *     sites   S = n_sites offsets t_s = offsets[site_first .. +S) along the guest's axis, 1 <= S <= PW_RIGID_MAX_SITES,
 *             each finite with |t_s| <= 16;
 *     rows    (A, B, C) per (site, atom), coef[coef_first + s*n + a], three doubles a row: 0 <= A, B <= 1e100, C finite
 *             with |C| <= 1e100 (C = q_a q_s / (4 pi eps_0) in the caller's units);
 *     charged 0 or 1: with 0 the column C is neither read nor evaluated;
 *     dirs    M = n_dirs directions dirs[dir_first .. +M), 1 <= M <= PW_RIGID_MAX_DIRS, three doubles each, every
 *             component finite and within [-1, 1].  The directions are data: nothing normalises them or checks their
 *             length;
 *     map_level  -1, or 0 <= map_level < L together with map_first >= 0.
 * POSE (v, o).  Voxel v has the centre (x, y, z) as in pw_cavity; orientation o the direction (dx, dy, dz).  Site s sits
 * at px = x + (t_s * dx), likewise py and pz: the product is rounded, then the sum; no contraction.  Per site the atoms
 * go in index order: r2 as in pw_affinity from (px - X, py - Y, pz - Z); the POSE is BLOCKED iff r2 <= core2 for any
 * (site, atom); an atom COUNTS for a site iff cutoff2 == 0.0 or r2 <= cutoff2; for a counting atom u is pw_affinity's
 * pair term from (A, B) and, when charged, u = u + C / sqrt(r2), the square root and the division correctly rounded;
 * U_s = U_s + u from +0.0.  The pose's energy is U = U_0, then U = U + U_s for s = 1 .. S-1.
 * WEIGHT.  Per beta and pose that is not blocked: w as in pw_affinity's WEIGHT from (beta, U), the clamp at 700 and
 * PW_AFF_CLAMPED in the job's flags included; the terms are z = w and e = w * U.
 * VOXEL.  Per beta zs = +0.0 and es = +0.0; for o = 0 .. M-1 in order zs = zs + z and es = es + e, blocked poses
 * skipped; zbar = zs * inv_M and ebar = es * inv_M with inv_M = 1.0 / (double)M.  umin_v is the smallest U of the
 * voxel's poses that are not blocked, by strict < in o order, +inf without one.  A voxel whose poses are all blocked is
 * DEAD.
 * SUMS.  Exactly pw_affinity's SUMS on the slots zbar and ebar: ranks by (l, j, i), chunks of 64 ranks, the tree k = 1,
 * 2, 4, 8, 16, 32, the chunk sums added in chunk order from +0.0; no floating-point atomics.  FP64 without contraction in
 * the association written: the same bytes on every device, launch geometry and run and on a device == -1 context.
 * Written: row `out` (n_voxels, n_blocked_poses, n_dead, u_min -- the smallest pose energy, ties to the lowest rank
 * and then the lowest o; +inf with min_voxel = min_dir = -1 without one --, min_voxel = (i, j, l), min_dir = o, the
 * flags); rows levels[level_first + b] = (Z_b, E_b), the totals of zbar and ebar; and, when map_level >= 0, per rank
 * the two doubles maps[map_first + 2*rank] = zbar at that level and maps[map_first + 2*rank + 1] = umin_v.
 * With S = 1, t_0 = 0, M = 1 and charged = 0 every output shared with pw_affinity is pw_affinity's bytes.
 * All pointers are host memory; n_points, n_coef, n_offsets, n_dirs, n_words, n_betas, n_maps, n_levels and n_out are
 * the rows of xyz, of coef (three doubles) and the entries of offsets, the rows of dirs, the entries of words, betas
 * and maps (doubles), the rows of levels and of out.  Jobs may share every input but no row of out or of levels and no
 * entry of maps; entries no job owns are never touched.  What is refused, and how, is as in pw_affinity
 * (PW_E_BAD_ARG, pw_last_error names the job -- of two that share, the later -- and the reason; nothing is launched
 * or written). */
#define PW_RIGID_MAX_SITES 8
#define PW_RIGID_MAX_DIRS 1024
typedef struct pw_rigid_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t coef_first;             /* rows (A, B, C) = coef[coef_first .. + n_sites*n), row s*n + a */
    int64_t word_first;             /* the region = words[word_first .. + ny*nz), or -1: every voxel */
    int64_t beta_first, n_betas;    /* betas[beta_first .. +n_betas) */
    int64_t site_first, n_sites;    /* offsets[site_first .. +n_sites) */
    int64_t dir_first, n_dirs;      /* dirs[dir_first .. +n_dirs), rows of three */
    int64_t level_first;            /* levels[level_first .. +n_betas) is written */
    int64_t map_first;              /* maps[map_first .. + 2*V) is written when map_level >= 0 */
    int64_t out;                    /* the job's row of out */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  spacing;                /* h > 0 */
    double  core2;                  /* >= 1e-6 */
    double  cutoff2;                /* 0.0: none; otherwise > core2 */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t charged;                /* 0 or 1 */
    int32_t map_level;              /* -1: no map; otherwise the beta whose zbar is written */
    int32_t reserved;               /* padding to a multiple of 8 bytes; not read */
} pw_rigid_job;
typedef struct pw_rigid_out {
    int64_t n_voxels, n_blocked_poses, n_dead;
    double  u_min;
    int32_t min_voxel[3];           /* (i, j, l), or -1 */
    int32_t min_dir;                /* o, or -1 */
    int32_t flags;                  /* PW_AFF_* */
    int32_t reserved;               /* padding to a multiple of 8 bytes; written as 0 */
} pw_rigid_out;
int pw_rigid_affinity(pw_context *ctx, const pw_rigid_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
                      const double *coef, int64_t n_coef, const double *offsets, int64_t n_offsets, const double *dirs,
                      int64_t n_dirs, const uint64_t *words, int64_t n_words, const double *betas, int64_t n_betas,
                      double *maps, int64_t n_maps, pw_affinity_level *levels, int64_t n_levels, pw_rigid_out *out,
                      int64_t n_out);
/* ---- rigid non-linear guests (H2O, CH4, SF6): pose tables ---------------------------------------------------------
 * pw_rigid_affinity for a guest that is a rigid body, not a line.  The text of record is
 * pywindow_amd/csrc/pw_rigid_body.hpp; in short, job k is a pw_rigid_affinity job without offsets and directions.  It
 * carries a pose table instead: M * S rows of three doubles poses[pose_first .. + n_dirs*n_sites), M = n_dirs,
 * S = n_sites, 1 <= M <= PW_RIGID_MAX_DIRS, 1 <= S <= PW_RIGID_MAX_SITES; row o*S + s is the displacement of site s
 * from the guest's centre in pose o, every component finite with |component| <= 16.  The rows are data: nothing
 * orthogonalises, checks or rotates them.
 * POSE (v, o).  Site s sits at px = x + p.x, likewise py and pz: one rounded sum a coordinate.  Everything after that
 * -- the pair term, charged or not, BLOCKED, COUNTS, the per-site accumulators, WEIGHT, VOXEL, SUMS and what is written
 * -- is pw_rigid_affinity's word for word; min_dir of the row of out is the pose index o.
 * With the table p = (t_s * dx, t_s * dy, t_s * dz), one rounded product each, every output is pw_rigid_affinity's
 * bytes for the offsets t and the directions d.  The same bytes on every device, launch geometry and run and on a
 * device == -1 context.
 * All pointers are host memory; n_pose_rows is the rows of poses (three doubles), the other counts are
 * pw_rigid_affinity's.  Refused (PW_E_BAD_ARG, pw_last_error reads "pw_rigid_body_affinity: job k: ..." and names
 * the later of two jobs that share; nothing is launched or written): what pw_rigid_affinity refuses of the fields the
 * two share, poses outside their array, and a pose component that is not finite or beyond 16. */
typedef struct pw_rigid_body_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t coef_first;             /* rows (A, B, C) = coef[coef_first .. + n_sites*n), row s*n + a */
    int64_t word_first;             /* the region = words[word_first .. + ny*nz), or -1: every voxel */
    int64_t beta_first, n_betas;    /* betas[beta_first .. +n_betas) */
    int64_t pose_first;             /* poses[pose_first .. + n_dirs*n_sites), rows of three, row o*n_sites + s */
    int64_t n_sites, n_dirs;        /* S and M */
    int64_t level_first;            /* levels[level_first .. +n_betas) is written */
    int64_t map_first;              /* maps[map_first .. + 2*V) is written when map_level >= 0 */
    int64_t out;                    /* the job's row of out */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  spacing;                /* h > 0 */
    double  core2;                  /* >= 1e-6 */
    double  cutoff2;                /* 0.0: none; otherwise > core2 */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t charged;                /* 0 or 1 */
    int32_t map_level;              /* -1: no map; otherwise the beta whose zbar is written */
    int32_t reserved;               /* padding to a multiple of 8 bytes; not read */
} pw_rigid_body_job;
int pw_rigid_body_affinity(pw_context *ctx, const pw_rigid_body_job *jobs, int64_t n_jobs, const double *xyz,
                           int64_t n_points, const double *coef, int64_t n_coef, const double *poses,
                           int64_t n_pose_rows, const uint64_t *words, int64_t n_words, const double *betas,
                           int64_t n_betas, double *maps, int64_t n_maps, pw_affinity_level *levels, int64_t n_levels,
                           pw_rigid_out *out, int64_t n_out);
/* ---- rigid linear guests in a crystal: the orientation-averaged Boltzmann factor over a periodic cell --------------
 * pw_rigid_affinity's pose, weight and fold at every voxel of the skewed grid of a periodic cell, so that the free energy
 * -ln(zbar) / beta of a rigid guest's centre can feed pw_percolation and pw_basins as a caller's field.  The reference
 * has no counterpart.  The text of record, with the proof of the atom skip, is pywindow_amd/csrc/pw_rigid_cell.hpp; in
 * short, job k has
 *     the grid of a pw_percolation job (origin, step, nx, ny, nz; the same voxel centres and ranks (l*ny + j)*nx + i);
 *     n >= 0 atoms xyz[atom_first .. +n), every periodic image that matters listed as an atom of its own;
 *     core2 >= 1e-6 and cutoff2 > core2; cutoff2 == 0 is refused: a cell has no "no cutoff";
 *     L = n_betas betas, S = n_sites offsets and M = n_dirs directions exactly as a pw_rigid_affinity job;
 *     rows (A, B) per (site, atom), coef[coef_first + s*n + a], TWO doubles a row: uncharged only.
 * POSE, WEIGHT, VOXEL and SUMS are pw_rigid_affinity's with charged = 0, the voxel centre being the cell grid's and
 * every voxel of the grid a rank.  Written: row `out` (pw_rigid_out: n_voxels = nx*ny*nz, n_blocked_poses, n_dead, u_min
 * with min_voxel and min_dir, ties to the lowest rank and then the lowest o; the flags); rows levels[level_first + b] =
 * (Z_b, E_b); and, when map_first >= 0, L + 1 planes of nx*ny*nz doubles from maps[map_first]: zbar at beta 0 .. L-1,
 * then umin_v (+inf at a dead voxel).  With S = 1, t_0 = 0, M = 1 the umin_v plane is pw_percolation's map byte for
 * byte; with step = (h, 0, h, 0, 0, h) every output shared with pw_rigid_affinity over the whole grid with the same
 * cutoff2 is that entry's bytes.  An atom that no pose of a block of 4 x 4 x 4 voxels can have within the cutoff is
 * left out for that block by a test that is proved conservative in floating point: the same bytes on every device,
 * launch geometry and run and on a device == -1 context, which may or may not skip.
 * All pointers are host memory; the counts are the rows of xyz, of coef (two doubles) and the entries of offsets, the
 * rows of dirs, the entries of betas and maps (doubles), the rows of levels and of out.  Jobs may share every input but
 * no row of out or of levels and no entry of maps; entries no job owns are never touched.  Refused (PW_E_BAD_ARG,
 * pw_last_error reads "pw_rigid_cell: job k: ..." and names the later of two jobs that share; nothing is launched or
 * written): what pw_percolation refuses of a grid, pw_rigid_affinity of sites, directions, betas and rows, cutoff2 == 0
 * or <= core2, more than 2^31 - 1 atoms, a range outside an array, shared outputs. */
typedef struct pw_rigid_cell_job {
    int64_t atom_first, n;          /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t coef_first;             /* rows (A, B) = coef[coef_first .. + n_sites*n), row s*n + a */
    int64_t beta_first, n_betas;    /* betas[beta_first .. +n_betas) */
    int64_t site_first, n_sites;    /* offsets[site_first .. +n_sites) */
    int64_t dir_first, n_dirs;      /* dirs[dir_first .. +n_dirs), rows of three */
    int64_t level_first;            /* levels[level_first .. +n_betas) is written */
    int64_t map_first;              /* maps[map_first .. + (n_betas + 1)*nx*ny*nz) is written, or -1: no maps */
    int64_t out;                    /* the job's row of out */
    double  origin[3];              /* the centre of voxel (0, 0, 0) */
    double  step[6];                /* ax, bx, by, cx, cy, cz */
    double  core2;                  /* >= 1e-6 */
    double  cutoff2;                /* > core2 */
    int32_t nx, ny, nz;             /* 1 .. PW_CAVITY_MAX_G */
    int32_t reserved;               /* padding to a multiple of 8 bytes; not read */
} pw_rigid_cell_job;
int pw_rigid_cell(pw_context *ctx, const pw_rigid_cell_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
                  const double *coef, int64_t n_coef, const double *offsets, int64_t n_offsets, const double *dirs,
                  int64_t n_dirs, const double *betas, int64_t n_betas, double *maps, int64_t n_maps,
                  pw_affinity_level *levels, int64_t n_levels, pw_rigid_out *out, int64_t n_out);
/* ---- charged rigid guests in a crystal: pw_rigid_cell with the Ewald sum of the framework's point charges ----------
 * The same field for a guest whose sites carry charges, against a framework of point charges: a defined periodic
 * electrostatic energy, which a cutoff Coulomb sum over images is not.  The reference has no counterpart.  The text of
 * record is pywindow_amd/csrc/pw_ewald.hpp; in short, job k is a pw_rigid_cell job (`cell`) whose rows of coef are
 * (A, B, C), THREE doubles a row, C = coulomb * q_site * q_atom in kJ/mol Angstrom, and which has
 *     charged (0 or 1): with 0 the job is pw_rigid_cell's definition verbatim and returns that entry's bytes; C, alpha,
 *     the site charges, the cell atoms and the rows are neither read nor evaluated;
 *     alpha >= 0, finite, the splitting parameter in 1 / Angstrom;
 *     S = cell.n_sites site charges site_q[charge_first .. +S);
 *     n_cell >= 0 cell atoms cell[cell_first .. +n_cell), rows (x, y, z, q) of four doubles: the atoms of the primary
 *     cell only, in the job's triangular frame, with their charges.  They make the structure factors; the listed atoms
 *     xyz with their images make the real-space part;
 *     K = n_k rows kvecs[k_first .. +K), 0 <= K <= PW_EWALD_MAX_K, rows (h, k, l, w) of four doubles: integer-valued
 *     indices of a reciprocal-lattice vector with |h|, |k|, |l| <= PW_EWALD_MAX_INDEX, and its weight w in kJ/mol per
 *     squared charge.  The rows are data, as the directions are: nothing derives or orders them.
 * A counting atom of a charged job adds (C * erfc(alpha * r)) / r to pw_rigid_cell's pair term, truncated at cutoff2 as
 * that term is; a pose's energy is the sum over its sites and then, last, Urec(v, o) = sum_k (P_ok cos(k . x_v) + Q_ok
 * sin(k . x_v)) in row order, with P and Q from the structure factors of the cell atoms and the form factors of the
 * guest in that orientation.  erfc is the library's own (pw_math.hpp: pw_erfc), exactly 1.0 at 0: with alpha == 0 and
 * K == 0 on a cell with step = (h, 0, h, 0, 0, h) every output shared with a charged pw_rigid_affinity job over the whole
 * grid is that entry's bytes.  Everything written, the skip of far atoms and the equality of the bytes on every device,
 * launch geometry, grouping and on a device == -1 context are pw_rigid_cell's.  Left out by design: the guest's
 * interaction with its own images (infinite dilution); any self or background term (none arises between a guest and a
 * NEUTRAL framework; neutrality is the caller's to ensure); non-linear guests.  The charges are given: pw_charges_cell
 * below makes them for a cell.
 * The counts are pw_rigid_cell's (coef: rows of three doubles) and the entries of site_q, the rows of cell and of kvecs.
 * Refused (PW_E_BAD_ARG, pw_last_error reads "pw_rigid_cell_ewald: job k: ..."; nothing is launched or written): what
 * pw_rigid_cell refuses; charged neither 0 nor 1; and of a charged job a charge term C, alpha, a site charge, a cell
 * atom or a weight that is not finite, alpha < 0, n_k outside 0 .. PW_EWALD_MAX_K, an index that is not an integer within
 * the cap, a range outside its array. */
#define PW_EWALD_MAX_K 4096
#define PW_EWALD_MAX_INDEX 64
typedef struct pw_rigid_cell_ewald_job {
    pw_rigid_cell_job cell;         /* the pw_rigid_cell job; rows (A, B, C) = coef[coef_first .. + n_sites*n) */
    int64_t charge_first;           /* site charges = site_q[charge_first .. + cell.n_sites) */
    int64_t cell_first, n_cell;     /* cell atoms = cell[cell_first .. +n_cell), rows (x, y, z, q) */
    int64_t k_first, n_k;           /* rows (h, k, l, w) = kvecs[k_first .. +n_k) */
    double  alpha;                  /* >= 0 */
    int32_t charged;                /* 0 or 1 */
    int32_t reserved;               /* padding to a multiple of 8 bytes; not read */
} pw_rigid_cell_ewald_job;
int pw_rigid_cell_ewald(pw_context *ctx, const pw_rigid_cell_ewald_job *jobs, int64_t n_jobs, const double *xyz,
                        int64_t n_points, const double *coef, int64_t n_coef, const double *offsets, int64_t n_offsets,
                        const double *dirs, int64_t n_dirs, const double *betas, int64_t n_betas, const double *site_q,
                        int64_t n_site_q, const double *cell, int64_t n_cell, const double *kvecs, int64_t n_kvecs,
                        double *maps, int64_t n_maps, pw_affinity_level *levels, int64_t n_levels, pw_rigid_out *out,
                        int64_t n_out);
/* ---- partial charges of an isolated molecule: charge equilibration ---------------------------------------------
 * The framework charges that the charged jobs of pw_rigid_affinity need, frame by frame, so that a breathing cage
 * gets the charges of each of its shapes: QEq (Rappe and Goddard 1991) with Ohno-Klopman shielding instead of Slater
 * overlap integrals.  The reference has no counterpart.  Job k has the n atoms xyz[xyz_first .. +n) (rows of three
 * doubles, Angstrom) with the parameters params[param_first .. +n) (rows (chi, J) in eV; jobs may share rows, the
 * frames of a trajectory share one set).  The charges minimise sum chi_i q_i + 1/2 q^T A q at sum q = total_charge,
 * with A_ii = J_i and A_ij = coulomb / sqrt(r_ij^2 + a^2), a = 2 coulomb / (J_i + J_j): one symmetric positive-definite
 * n x n problem, solved as A s = -chi and A t = 1 by Jacobi-preconditioned conjugate gradients that stop at a relative
 * residual of tol or after max_iter steps, then q = s + mu t with mu = (total_charge - sum s) / sum t.  The charges go
 * to charges[charge_first .. +n); row `out` of the result holds mu (the equalised electronegativity, eV), the two
 * sums, energy = (chi.q + mu total_charge) / 2 (eV), the dipole sum q_i x_i (e Angstrom), the extreme charges, the
 * steps of the two systems and flags: PW_CHG_NOT_CONVERGED (max_iter reached; the charges of the last step are
 * written), PW_CHG_BREAKDOWN (a direction of no positive curvature: the matrix is not positive definite to working
 * precision) and PW_CHG_NO_SUM (sum t is not positive).  With one of the last two the charges, mu, energy, dipole,
 * q_min and q_max are NaN: a result, not an error.
 * The result is DEFINED (pywindow_amd/csrc/pw_charges.hpp: the sums of pw_superpose, every step of the solver written
 * out): the same bits on every device, launch geometry and run and on a device == -1 context (host threads),
 * whatever else shares the call, wherever a job's vectors live (LDS up to 512 atoms, a workspace beyond) and however
 * the jobs are cut into launches to bound that workspace.  A NaN always leaves as 0x7ff8000000000000.
 * All pointers are host memory; n_points is the number of rows of xyz, of rows of params and of entries of charges.
 * Jobs may share neither rows of `out` nor entries of `charges`; what no job owns is never touched.  n < 1, a range
 * outside the arrays, a coordinate, chi, J, total_charge or coulomb that is not finite, J <= 0, coulomb <= 0, tol
 * outside [1e-14, 1e-2] or max_iter outside [1, 100000]: PW_E_BAD_ARG (pw_last_error names the job and the reason),
 * and nothing is launched or written.  Device work is queued on the context's stream, its memory allocated and freed
 * in stream order; the call returns when the results are in place. */
#define PW_CHG_NOT_CONVERGED 1
#define PW_CHG_BREAKDOWN 2
#define PW_CHG_NO_SUM 4
typedef struct pw_charges_job {
    int64_t xyz_first;       /* first row of xyz */
    int64_t param_first;     /* first row of params */
    int64_t n;               /* atoms, >= 1 */
    double  total_charge;    /* Q, e */
    double  coulomb;         /* K, eV Angstrom: 14.399645... for charges in e */
    double  tol;             /* relative residual at which a system stops, in [1e-14, 1e-2] */
    int64_t max_iter;        /* in [1, 100000] */
    int64_t charge_first;    /* first entry of charges */
    int64_t out;             /* the job's row of the result */
} pw_charges_job;
typedef struct pw_charges_out {
    double  mu;
    double  sum_s, sum_t;
    double  energy;
    double  dipole[3];
    double  q_min, q_max;
    int32_t iterations[2];   /* of A s = -chi and of A t = 1 */
    int32_t flags;           /* PW_CHG_* */
    int32_t reserved;        /* padding to a multiple of 8 bytes; written as 0 */
} pw_charges_out;
int pw_charges(pw_context *ctx, const pw_charges_job *jobs, int64_t n_jobs, const double *xyz, const double *params,
               int64_t n_points, double *charges, pw_charges_out *out);
/* ---- partial charges of a periodic crystal cell: charge equilibration with an Ewald sum ------------------------------
 * pw_charges treats a cage as if it sat in vacuum; this entry makes the charges that pw_rigid_cell_ewald needs for the
 * cell itself.  The reference has no counterpart.  The text of record is pywindow_amd/csrc/pw_charges_cell.hpp; in
 * short, job k has the n >= 1 atoms xyz[xyz_first .. +n) in the triangular frame of the cell's edges (a1, b1, b2, c1, c2,
 * c3), taken as they are (the caller wraps them into the cell), the parameters params[param_first .. +n) (rows (chi, J)
 * in eV), coulomb in eV Angstrom, alpha >= 0 in 1 / Angstrom, cutoff2, the switch shield_on2 < shield_off2 <= cutoff2
 * (Angstrom^2), and n_k rows kvecs[k_first .. +n_k) (h, k, l, w): the rows of pw_rigid_cell_ewald with the weight in eV
 * per squared charge, data as they are there, under the same caps.  The cell is neutral: there is no total charge.
 * The charges minimise sum chi_i q_i + 1/2 q^T A q at sum q = 0 with A = D + R + G: D_i = J_i - coulomb 2 alpha / sqrt(pi);
 * R the sum over the 27 nearest images (an atom's own included, itself not) within cutoff2, equality counting, of
 * s(r2) (K / sqrt(r2 + a^2) - K / r) + K erfc(alpha r) / r with a = 2 K / (J_i + J_j) and s the quintic switch that is 1
 * below shield_on2 and 0 above shield_off2 (coincident atoms take the finite limit); G_ij = sum_k w_k cos(k . (x_i -
 * x_j)), applied through structure factors.  Twenty-seven images suffice for wrapped atoms when the cutoff is at most
 * the cell's smallest perpendicular width; the entry checks neither.  The solver is projected, Jacobi-preconditioned
 * conjugate gradients on the neutral subspace; it stops at rz <= tol^2 rz0 or after max_iter steps.  The charges go to
 * charges[charge_first .. +n); row `out` holds mu (the equalised electronegativity, eV), energy = chi.q / 2 (eV), the
 * extreme charges, the steps and flags with pw_charges' meanings (PW_CHG_NOT_CONVERGED: the charges of the last step are
 * written; PW_CHG_BREAKDOWN and PW_CHG_NO_SUM: everything but the steps and flags is NaN).  There is no dipole.
 * The result is DEFINED: the same bits on every device, launch geometry and run and on a device == -1 context, whatever
 * else shares the call, wherever a job's vectors live (LDS up to 1536 atoms, a workspace beyond), whether a row of R is
 * stored or recomputed and however the jobs are cut into launches.  A NaN always leaves as 0x7ff8000000000000.
 * All pointers are host memory; n_points is the number of rows of xyz, of rows of params and of entries of charges,
 * n_kvecs the rows of kvecs.  Refused (PW_E_BAD_ARG, pw_last_error reads "pw_charges_cell: job k: ..."; nothing is
 * launched or written): n < 1, a range outside its array, shared rows of out or entries of charges, a value that is not
 * finite, J <= 0, coulomb <= 0, alpha < 0, cutoff2 <= 0, shield_on2 < 0, shield_on2 >= shield_off2, shield_off2 >
 * cutoff2, a1, b2 or c3 not positive, n_k outside 0 .. PW_EWALD_MAX_K, an index that is not an integer within
 * PW_EWALD_MAX_INDEX, tol outside [1e-14, 1e-2], max_iter outside [1, 100000]. */
typedef struct pw_charges_cell_job {
    int64_t xyz_first;       /* first row of xyz */
    int64_t param_first;     /* first row of params */
    int64_t n;               /* atoms, >= 1 */
    int64_t k_first, n_k;    /* rows (h, k, l, w) = kvecs[k_first .. +n_k) */
    double  edges[6];        /* a1, b1, b2, c1, c2, c3 */
    double  coulomb;         /* K, eV Angstrom */
    double  alpha;           /* >= 0 */
    double  cutoff2;         /* > 0 */
    double  shield_on2, shield_off2;
    double  tol;             /* in [1e-14, 1e-2] */
    int64_t max_iter;        /* in [1, 100000] */
    int64_t charge_first;    /* first entry of charges */
    int64_t out;             /* the job's row of the result */
} pw_charges_cell_job;
typedef struct pw_charges_cell_out {
    double  mu;
    double  energy;
    double  q_min, q_max;
    int32_t iterations;
    int32_t flags;           /* PW_CHG_* */
} pw_charges_cell_out;
int pw_charges_cell(pw_context *ctx, const pw_charges_cell_job *jobs, int64_t n_jobs, const double *xyz,
                    const double *params, int64_t n_points, const double *kvecs, int64_t n_kvecs, double *charges,
                    pw_charges_cell_out *out);
/* ---- the pore network of a crystal cell: periodic void components and in how many dimensions each percolates ----
 * Every grid entry above looks at one cage cut out of its surroundings.  This one takes a whole periodic cell: are
 * its voids connected, in how many dimensions, for a guest of which size, and how much of the void is accessible
 * through that network rather than locked in pockets.  The reference has no counterpart.  The text of record, with the
 * proofs, is pywindow_amd/csrc/pw_channels.hpp; in short, job k (one cell at one probe) has
 *     atoms   n >= 0 atoms xyz[atom_first .. +n) with radii[radius_first .. +n) and a probe >= 0.  The job lists every
 *             periodic image that matters as an atom of its own: only the fill wraps, not the classification;
 *     a grid  nx x ny x nz voxels, each 1 .. PW_CAVITY_MAX_G, an origin o and step = (ax, bx, by, cx, cy, cz): the cell's
 *             first vector along x, its second in the xy plane; ax, by, cz > 0.  Voxel (i, j, l) has the centre
 *             z = oz + (double)l*cz, y = (oy + (double)j*by) + (double)l*cy,
 *             x = ((ox + (double)i*ax) + (double)j*bx) + (double)l*cx  (products rounded, sums left to right, no fma).
 * A voxel is OPEN iff it is free by pw_cavity's test (equality is free); there are no planes.  Voxel v has the six
 * neighbours v +- e_k with indices mod n_k; a step +e_k from index n_k - 1 or -e_k from index 0 CROSSES face k.  The
 * COMPONENTS are the connected components of the open voxels, numbered by their first voxel in rank
 * (l * ny + j) * nx + i ascending.  For phi in 1 .. 7 (bit 0 = a, 1 = b, 2 = c), on the nodes (voxel, parity) where a
 * step changes parity iff it crosses a face of phi, bit phi - 1 of a component's `wraps` is set iff (first voxel, 1)
 * is reachable from (first voxel, 0): iff the component holds a closed path whose winding vector w has phi . w odd.
 * rank = 3 - log2(1 + number of clear bits) is the rank mod 2 of the winding lattice: 0 a pocket, 1 a channel, 2 a
 * layer, 3 a network.  LIMIT: a component all of whose winding vectors are even (a double helix of pitch two cells)
 * reads as a pocket.
 * Row `out` of the result: n_open, n_components (all of them), n_recorded = min(n_components, c_max), the voxels and
 * the components by rank over ALL components (sum n_voxels_by_rank == n_open), flags (PW_CHAN_TRUNCATED iff
 * n_components > c_max).  Rows comps[comp_first .. + c_max): the first n_recorded components -- first (the rank of the
 * first voxel), n_voxels, n_cross[k] (its voxels at index n_k - 1 whose +e_k neighbour is in it), wraps, rank -- and
 * the rest of the c_max rows written as first = -1 and zeros.  mask_first >= 0: the ACCESSIBLE words, the OR of every
 * component of rank >= 1, to mask[mask_first .. + ny*nz) in the layout of pw_cavity's mask (so they serve as `words`
 * of pw_affinity and pw_sasa).  label_first >= 0: one byte a voxel in rank order to labels[label_first .. + nx*ny*nz):
 * the component's row index, 254 for a component beyond c_max, 255 for a voxel that is not open.
 * Every output is an integer, so the bytes are this definition on every device, launch geometry and run and on a
 * device == -1 context.  Jobs may share atoms and radii but no output; entries no job owns are never touched.  A value
 * a job reads that is not finite, ax, by or cz <= 0, a negative radius or probe, a dimension outside
 * 1 .. PW_CAVITY_MAX_G, c_max outside 0 .. PW_CHAN_MAX_COMPONENTS, a range outside an array or jobs that share
 * outputs (the later of the two is named): PW_E_BAD_ARG, and nothing is launched or written. */
#define PW_CHAN_MAX_COMPONENTS 254
#define PW_CHAN_TRUNCATED 1      /* more components than c_max: the table holds the first c_max, the totals all */
typedef struct pw_channels_job {
    int64_t atom_first, n;      /* atoms = xyz[atom_first .. +n), n >= 0 */
    int64_t radius_first;       /* their radii = radii[radius_first .. +n) */
    int64_t comp_first;         /* comps[comp_first .. + c_max) is written */
    int64_t mask_first;         /* mask[mask_first .. + ny*nz) is written, or -1: no mask */
    int64_t label_first;        /* labels[label_first .. + nx*ny*nz) is written, or -1: no labels */
    int64_t out;                /* the job's row of the result */
    double  origin[3];          /* the centre of voxel (0, 0, 0) */
    double  step[6];            /* ax, bx, by, cx, cy, cz */
    double  probe;              /* >= 0 */
    int32_t nx, ny, nz;         /* 1 .. PW_CAVITY_MAX_G */
    int32_t c_max;              /* 0 .. PW_CHAN_MAX_COMPONENTS */
} pw_channels_job;
typedef struct pw_channels_comp {
    int64_t first;              /* the rank of the component's first voxel; -1 in a row beyond n_recorded */
    int64_t n_voxels;
    int64_t n_cross[3];
    int32_t wraps;              /* bit phi - 1, phi in 1 .. 7 */
    int32_t rank;               /* 0 .. 3 */
} pw_channels_comp;
typedef struct pw_channels_out {
    int64_t n_open, n_components, n_recorded;
    int64_t n_voxels_by_rank[4];
    int64_t n_components_by_rank[4];
    int32_t flags;              /* PW_CHAN_* */
    int32_t reserved;           /* padding to a multiple of 8 bytes; written as 0 */
} pw_channels_out;
int pw_channels(pw_context *ctx, const pw_channels_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
                const double *radii, int64_t n_radii, pw_channels_out *out, int64_t n_out, pw_channels_comp *comps,
                int64_t n_comps, uint64_t *mask, int64_t n_mask, uint8_t *labels, int64_t n_labels);
/* ---- guest percolation: the energy levels at which the voids of a crystal cell connect ---------------------------
 * pw_channels answers the hard-sphere question; what lets a guest through a soft wall is the energy barrier.  For one
 * guest in one periodic cell this entry finds, for each of six connection criteria, the lowest energy level at which
 * the sub-level set of the guest's energy landscape holds a component that meets the criterion: the minimax
 * (bottleneck) barrier of diffusion.  The reference has no counterpart.  The text of record, with the proofs, is
 * pywindow_amd/csrc/pw_percolate.hpp; in short, job k has
 *     the grid of pw_channels (nx, ny, nz, origin, step; the same centres, neighbours and face crossings);
 *     a field U over every voxel in rank (l*ny + j)*nx + i: with field_first == -1 the Lennard-Jones energy of the
 *             atoms xyz[atom_first .. +n) with rows (A, B) = coef[coef_first .. +n), core2 and cutoff2, exactly as
 *             pw_passage computes it (+inf at a blocked voxel; the job lists every periodic image that matters as an
 *             atom of its own); with field_first >= 0 the caller's field[field_first .. + nx*ny*nz), every value finite
 *             or +inf.  map_first >= 0: the field is also written to map[map_first .. + nx*ny*nz).
 * allowed_t(v): U_v is not +inf and U_v <= t.  Criterion c = 0, 1, 2: some periodic component of allowed_t has
 * rank >= 1, 2, 3 (pw_channels' rank); c = 3, 4, 5: some component has the bit of phi = 1, 2, 4 of its wraps set (a
 * closed path that winds an odd number of times along a, b, c).  Each is monotone in t and changes only at voxel values.
 * Row `out` of the result: n_blocked, u_min with u_min_voxel (the lowest rank on a tie; +inf and -1 without a finite
 * voxel) and flags (PW_PERC_NEVER iff criterion 0 never holds).  Rows levels[level_first .. + 6), one a criterion:
 * level = B_c, the smallest voxel value at which the criterion holds (+inf with PW_PERC_NEVER when it does not hold at
 * the largest finite value); first, n_voxels, wraps, rank of the component C of allowed_{B_c} that meets the criterion
 * and has the lowest first voxel; saddle, the voxel of C with U == B_c of the lowest rank (level carries the bits of U
 * there); well and well_voxel, the smallest U over C with ties to the lowest rank; n_allowed = |allowed_{B_c}|.  With
 * PW_PERC_NEVER: voxels and first -1, counts, wraps and rank 0, well +inf.
 * Every output is a comparison of doubles or an integer count over the defined field: the same bytes on every device,
 * launch geometry and run and on a device == -1 context.  LIMITS: pw_channels' (windings that are all even read as
 * none); one guest, no guest-guest term, no charges; the bottleneck of the grid's 6-connectivity at its spacing.
 * Jobs may share atoms, rows of coef and fields but no output; entries no job owns are never touched.  What pw_channels
 * refuses of a grid and pw_passage of atoms, coefficients, core2, cutoff2 and a field, a range outside an array or jobs
 * that share outputs (the later of the two is named): PW_E_BAD_ARG, and nothing is launched or written. */
#define PW_PERC_CRITERIA 6
#define PW_PERC_NEVER 1          /* the criterion holds at no finite level */
typedef struct pw_percolation_job {
    int64_t atom_first, n;      /* atoms = xyz[atom_first .. +n), n >= 0 (read when field_first == -1) */
    int64_t coef_first;         /* their rows (A, B) = coef[coef_first .. +n) */
    int64_t field_first;        /* -1: Lennard-Jones from the atoms; >= 0: field[field_first .. + nx*ny*nz) */
    int64_t map_first;          /* map[map_first .. + nx*ny*nz) is written, or -1: no map */
    int64_t level_first;        /* levels[level_first .. + 6) is written */
    int64_t out;                /* the job's row of the result */
    double  origin[3];          /* the centre of voxel (0, 0, 0) */
    double  step[6];            /* ax, bx, by, cx, cy, cz */
    double  core2;              /* >= 1e-6 */
    double  cutoff2;            /* 0.0: none; otherwise > core2 */
    int32_t nx, ny, nz;         /* 1 .. PW_CAVITY_MAX_G */
    int32_t reserved;           /* padding to a multiple of 8 bytes; not read */
} pw_percolation_job;
typedef struct pw_percolation_level {
    double  level;              /* B_c: the bits of U at the saddle, or +inf */
    double  well;
    int64_t first, n_voxels;    /* of the component C */
    int64_t n_allowed;
    int32_t saddle[3];          /* (i, j, l), or -1 */
    int32_t well_voxel[3];
    int32_t wraps, rank;        /* of C */
    int32_t flags;              /* PW_PERC_* */
    int32_t reserved;           /* padding to a multiple of 8 bytes; written as 0 */
} pw_percolation_level;
typedef struct pw_percolation_out {
    int64_t n_blocked;
    double  u_min;
    int32_t u_min_voxel[3];     /* (i, j, l), or -1 */
    int32_t flags;              /* PW_PERC_NEVER iff criterion 0 never holds */
} pw_percolation_out;
int pw_percolation(pw_context *ctx, const pw_percolation_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
                   const double *coef, int64_t n_coef, const double *field, int64_t n_field, double *map, int64_t n_map,
                   pw_percolation_level *levels, int64_t n_levels, pw_percolation_out *out, int64_t n_out);
/* ---- crystal diffusion: the energy basins of a cell, the dividing surfaces between them and their Boltzmann sums -----
 * pw_percolation gives the level at which the landscape connects; a rate needs how roomy the wells and how wide the
 * saddles are.  This entry cuts the landscape of one guest in one periodic cell into the basins of steepest descent on
 * the grid, with the integer cell offset of every voxel to its basin's root, and sums Boltzmann weights over every
 * basin and over every dividing surface between two basins (or a basin and its own periodic image); the hop network
 * and the diffusion tensor follow from the rows by plain linear algebra (pywindow_amd/diffusion.py).  The reference has
 * no counterpart.  The text of record, with the proofs, is pywindow_amd/csrc/pw_basins.hpp; in short, job k has
 *     pw_percolation's grid and field (atoms or field_first, map_first), n_betas = 1 .. 8 inverse temperatures
 *     betas[0 .. n_betas), each finite and > 0, and an energy cap (finite or +inf).
 * A voxel is allowed when U is not +inf and U <= cap.  Its parent is the first in (key(U), rank, position) of itself and
 * its allowed neighbours in the order -a, +a, -b, +b, -c, +c; roots are their own parents and are numbered 0 .. B-1 by
 * rank; o(v) is the sum of the face crossings along the parents from v to its root.  Row `out`: n_basins = B and
 * n_edges = E (the true counts), what was written of each, n_blocked (voxels at +inf), n_allowed, u_min with its voxel
 * over the allowed voxels (+inf and -1 without one) and flags.  basins[basin_first .. + min(B, b_cap)): root, n_voxels,
 * u_min (the root's bits), z[b] = sum of w = pw_exp(-(beta_b * U)) (the exponent clamped at 700 with PW_BAS_CLAMPED)
 * and e[b] = sum of w * U over the basin's voxels.  A face between allowed v and v' = v + e_k whose voxels differ in
 * basin, or in o beyond the face's own crossing, belongs to the edge (a, b, d) in canonical form (a <= b; a == b: the
 * first non-zero component of d positive); edges[edge_first .. + E), ascending in (a, b, d): n_faces, saddle (the
 * smallest face term max(U_v, U_v') by key) with saddle_voxel (v's rank) and saddle_k, and s[b][k] = the sum of
 * w(term) over the faces across e_k.  Every sum is taken in a written association (row chunks of 64 slots in
 * pw_affinity's tree, then rows in order), everything else is a comparison or an integer count: the same bytes on every
 * device, launch geometry, workspace budget and run and on a device == -1 context.  PW_BAS_OVERFLOW (B > b_cap or
 * E > e_cap): the first b_cap basins and no edge are written.  PW_BAS_RANGE (a component of an o(v) or a d beyond
 * +-PW_BAS_MAX_OFFSET): no edge is written, n_edges is 0, the o of the labels are 0.  labels[label_first .. + nx*ny*nz)
 * when label_first >= 0: basin (-1: not allowed) and o per voxel.  Rows beyond what was written are not touched.
 * Refusals as pw_percolation's, and b_cap or e_cap < 0, n_betas outside 1 .. 8, a beta that is not finite or not
 * positive, a cap that is not a number or -inf: PW_E_BAD_ARG, nothing launched or written. */
#define PW_BAS_MAX_BETAS 8
#define PW_BAS_MAX_OFFSET 255
#define PW_BAS_OVERFLOW 1        /* more basins than b_cap or more edges than e_cap */
#define PW_BAS_CLAMPED 2         /* an exponent was clamped at 700 */
#define PW_BAS_RANGE 4           /* a cell offset left +-PW_BAS_MAX_OFFSET */
typedef struct pw_basins_job {
    int64_t atom_first, n;      /* atoms = xyz[atom_first .. +n), n >= 0 (read when field_first == -1) */
    int64_t coef_first;         /* their rows (A, B) = coef[coef_first .. +n) */
    int64_t field_first;        /* -1: Lennard-Jones from the atoms; >= 0: field[field_first .. + nx*ny*nz) */
    int64_t map_first;          /* map[map_first .. + nx*ny*nz) is written, or -1: no map */
    int64_t basin_first;        /* basins[basin_first .. + b_cap) may be written */
    int64_t edge_first;         /* edges[edge_first .. + e_cap) may be written */
    int64_t label_first;        /* labels[label_first .. + nx*ny*nz) is written, or -1: no labels */
    int64_t out;                /* the job's row of the result */
    int64_t b_cap, e_cap;       /* >= 0 */
    double  origin[3];          /* the centre of voxel (0, 0, 0) */
    double  step[6];            /* ax, bx, by, cx, cy, cz */
    double  core2;              /* >= 1e-6 */
    double  cutoff2;            /* 0.0: none; otherwise > core2 */
    double  cap;                /* finite or +inf */
    double  betas[PW_BAS_MAX_BETAS];
    int32_t nx, ny, nz;         /* 1 .. PW_CAVITY_MAX_G */
    int32_t n_betas;            /* 1 .. PW_BAS_MAX_BETAS */
} pw_basins_job;
typedef struct pw_basins_basin {
    int64_t root, n_voxels;
    double  u_min;              /* the bits of U at the root */
    double  z[PW_BAS_MAX_BETAS], e[PW_BAS_MAX_BETAS];
} pw_basins_basin;
typedef struct pw_basins_edge {
    int32_t a, b, d[3];
    int32_t saddle_k;
    int64_t n_faces;
    int64_t saddle_voxel;       /* the rank of v of the saddle's face (v, saddle_k) */
    double  saddle;
    double  s[PW_BAS_MAX_BETAS][3];
} pw_basins_edge;
typedef struct pw_basins_label {
    int32_t basin;              /* -1: not allowed */
    int32_t o[3];
} pw_basins_label;
typedef struct pw_basins_out {
    int64_t n_basins, n_edges;  /* B and E */
    int64_t n_basins_written, n_edges_written;
    int64_t n_blocked, n_allowed;
    double  u_min;
    int32_t u_min_voxel[3];     /* (i, j, l), or -1 */
    int32_t flags;              /* PW_BAS_* */
} pw_basins_out;
int pw_basins(pw_context *ctx, const pw_basins_job *jobs, int64_t n_jobs, const double *xyz, int64_t n_points,
              const double *coef, int64_t n_coef, const double *field, int64_t n_field, double *map, int64_t n_map,
              pw_basins_basin *basins, int64_t n_basins, pw_basins_edge *edges, int64_t n_edges, pw_basins_label *labels,
              int64_t n_labels, pw_basins_out *out, int64_t n_out);

/* Native DL_POLY HISTORY ingest (trajectory.py:647-766): see pw_history_* in
 * pywindow_amd/csrc/pw_history.cpp */
typedef struct pw_history pw_history;
int pw_history_open(const char *path, pw_history **h);
int64_t pw_history_frames(const pw_history *h);
int64_t pw_history_atoms(const pw_history *h);
int pw_history_keytrj(const pw_history *h);
int pw_history_imcon(const pw_history *h);
/* atom keys of frame 0, NUL-separated, into buf (returns bytes needed) */
int64_t pw_history_atom_keys(const pw_history *h, char *buf, int64_t buflen);
/* coordinates of frames [first, first+count) -> xyz[count][natoms][3]; lattice[count][9] may be NULL */
int pw_history_read(const pw_history *h, int64_t first, int64_t count, double *xyz, double *lattice);
/* nstep and tstep of the "timestep" record of one frame (reference: frame_info, trajectory.py:712-721; natms,
 * keytrj and imcon of the record are the file's: pw_history_atoms / _keytrj / _imcon) */
int pw_history_frame_info(const pw_history *h, int64_t frame, int64_t *nstep, double *tstep);
/* host threads the reader decodes with (PW_READER_THREADS or the hardware concurrency, at most 16; they are
 * started once per process and parked between calls) */
int pw_history_reader_threads(void);
/* Frames [first_frame, first_frame + count) decoded into `staging` (count x natoms x 3, normally the context's
 * page-locked buffer: pw_context_pinned) and appended to the streamed batch `res` (pw_resident_stream_begin) as units
 * first_unit.. WHILE the decoding goes on: the reader's threads take blocks of frames, one more thread appends the
 * finished prefix whenever it has grown by min_append frames (<= 0: 64).  The frame loop of
 * Trajectory._analysis_serial (trajectory.py:496-522: read a frame, analyse it, read the next) with the reading and
 * the analysis side by side.  legs_ms (may be NULL): [0] ms until the last frame was decoded, [1] from there until the
 * last append had returned.  Called without holding anything: the appends take the context's mutex one at a time. */
int pw_history_stream_read(const pw_history *h, int64_t first_frame, int64_t count, pw_context *ctx, pw_resident *res,
                           int64_t first_unit, double *staging, int64_t min_append, double *legs_ms);
void pw_history_close(pw_history *h);

#ifdef __cplusplus
}
#endif
#endif /* PYWINDOW_AMD_H */
