/*
 * voxgraph_amd.h -- C ABI of libvoxgraph_amd.so: voxgraph's two data-parallel
 * inner loops as hand-written HIP kernels for MI355X (gfx950).
 *
 *   REG  : voxgraph::RegistrationCostFunction::Evaluate
 *          (voxgraph/src/backend/constraint/cost_functions/registration_cost_function.cpp:58-298)
 *   TSDF : voxblox::FastTsdfIntegrator::integratePointCloud, called at
 *          voxgraph/src/frontend/measurement_processors/pointcloud_integrator.cpp:83
 *
 * Plain C: opaque handles, pointers and sizes, int status codes.  No
 * exceptions or aborts cross this boundary.  All host pointers are ordinary
 * (pageable) memory unless a parameter is documented as a DEVICE pointer.
 * There is no CPU fallback: without a gfx950 device vgx_ctx_create fails with
 * VGX_ERR_NO_DEVICE and nothing else can be called.
 *
 * Reference citations are relative to /root/reference/voxgraph/.
 * INTEGRATION.md shows the reference-side C++ that binds these entry points.
 */
#ifndef VOXGRAPH_AMD_H_
#define VOXGRAPH_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGX_API __attribute__((visibility("default")))

/* ---- status codes ------------------------------------------------------ */
#define VGX_OK 0
/* Evaluate() would `return false`: summed reference weight == 0
 * (registration_cost_function.cpp:273).  Outputs are unspecified. */
#define VGX_EVALUATE_FALSE 1
#define VGX_ERR_INVALID (-1)     /* bad argument / handle / state            */
#define VGX_ERR_HIP (-2)         /* a HIP runtime call failed                */
#define VGX_ERR_NOMEM (-3)       /* host or device allocation failed         */
#define VGX_ERR_UNSUPPORTED (-4) /* e.g. voxels_per_side not in {8,16}       */
#define VGX_ERR_NO_DEVICE (-5)   /* no HIP device / not gfx950               */
#define VGX_ERR_NOT_POSITIVE_DEFINITE (-6) /* vgx_dense_spd_solve: a pivot that is not positive or not finite */

typedef struct vgx_ctx_s* vgx_ctx;
typedef struct vgx_submap_s* vgx_submap;
typedef struct vgx_reg_s* vgx_reg;
typedef struct vgx_reg_batch_s* vgx_reg_batch;
typedef struct vgx_reg_multi_s* vgx_reg_multi;
typedef struct vgx_reg_assembler_s* vgx_reg_assembler;

/* ---- context ----------------------------------------------------------- */
/* One context per process per GPU (one process per GPU is the multi-GPU
 * model; constraint shards meet in an RCCL all-reduce issued by the host on
 * the buffer vgx_reg_batch_evaluate_normal fills). */
VGX_API int vgx_ctx_create(int device, vgx_ctx* out);
VGX_API int vgx_ctx_destroy(vgx_ctx ctx);
/* Human-readable description of the last error on this context (or of the
 * last failed vgx_ctx_create when ctx == NULL). Never NULL. */
VGX_API const char* vgx_last_error(vgx_ctx ctx);
/* THREADING AND STREAMS.  A context has two sides, each with its own HIP stream and its own lock, as the reference has
 * two threads (voxgraph_mapper.cpp:218-238: the ROS thread integrates scans while optimizePoseGraph runs on a
 * std::async thread):
 *   registration side   everything on FINISHED submaps -- vgx_submap_*, vgx_reg_*, vgx_find_overlapping_pairs,
 *                       vgx_map_file_load_submap ...; stream: vgx_ctx_set_stream / _get_stream.
 *   TSDF side           the ACTIVE submap -- vgx_tsdf_layer_*, vgx_tsdf_integrator_*, vgx_tsdf_integrate*;
 *                       stream: vgx_ctx_set_tsdf_stream / _get_tsdf_stream.
 * A scan therefore neither queues behind a solver evaluation nor waits for its lock: one thread may integrate while
 * another evaluates, on the same context (tests/test_concurrency_gpu.py).  What makes that safe is the reference's own
 * invariant (voxgraph_mapper.cpp:464-471): a finished submap is immutable, and only the active layer is written.  The
 * two sides meet in vgx_submap_from_tsdf_layer (finishSubmap(), voxgraph_submap.cpp:84-107), which orders the
 * registration stream behind the TSDF stream with an event; the layer must not be integrated into while that call
 * runs (the reference finishes a submap on the thread that integrates).  Any entry point may be called from any
 * thread; calls on one side are serialised among themselves (except the drop-in vgx_reg_evaluate, which overlaps on up
 * to eight evaluation streams).  DEVICE pointers handed to vgx_tsdf_integrate*_device must be ready with respect to the
 * TSDF stream (complete, produced on / ordered before vgx_ctx_get_tsdf_stream(), or ordered behind their producer with
 * vgx_ctx_tsdf_wait_for_stream).  NOTE for callers that set the context's stream to their own (vgx_ctx_set_stream) and
 * produce scan points on it: since round 5 scans do NOT run on that stream -- order them with
 * vgx_ctx_tsdf_wait_for_stream(ctx, NULL) before the vgx_tsdf_integrate*_device call, or hand the same stream to
 * vgx_ctx_set_tsdf_stream as well.
 *
 * PRIORITY.  The TSDF side goes first: the context's own TSDF stream is created with the device's highest stream
 * priority and its own registration stream with the lowest, so that a scan (one short kernel the sensor's cadence waits
 * for) is dispatched as workgroups of a running solver evaluation (thousands, which nobody waits for one by one) retire
 * instead of behind all of them -- voxgraph optimises in the background of its mapping thread
 * (voxgraph_mapper.cpp:218-238).  Priorities alone did not do it on gfx950 (measured); what does: while the context has a
 * TSDF integrator, the fused pass's tile kernel is launched FIVE workgroups deep per CU instead of six, which leaves the
 * registers of one scan workgroup free on every CU -- a scan under a running solve then takes 0.14-0.32 ms (median)
 * instead of 0.7 ms, at + 3 % per solver evaluation; a context without an integrator runs the solver at full depth.
 * Measured per-scan latency under a running solve: bench.py `tsdf.*.latency_under_solve_us`,
 * profiles/r06_scan_latency.txt.  Streams handed in by the caller keep the priority
 * the caller gave them.  vgx_ctx_stream_priorities: 1 when the own streams were created that way (0: the device offers
 * one level only).
 *
 * vgx_ctx_set_stream: launch the registration side on an existing hipStream_t (e.g. the caller's PyTorch stream);
 * vgx_ctx_set_tsdf_stream: the same for the TSDF side (waits for what that side has queued so far).  NULL restores
 * the context's own stream.  vgx_ctx_synchronize waits for both, vgx_ctx_synchronize_tsdf for the TSDF side alone (the
 * mapping thread's "is my scan in?", whatever the solver has queued).  vgx_ctx_tsdf_wait_for_stream: the TSDF stream
 * waits ON THE DEVICE for what producer_stream (NULL: the context's registration stream) holds at the time of the call
 * (HIP's legacy default stream, whose handle IS NULL, cannot be named here: produce on a created stream). */
VGX_API int vgx_ctx_set_stream(vgx_ctx ctx, void* hip_stream);
VGX_API void* vgx_ctx_get_stream(vgx_ctx ctx);
VGX_API int vgx_ctx_set_tsdf_stream(vgx_ctx ctx, void* hip_stream);
VGX_API void* vgx_ctx_get_tsdf_stream(vgx_ctx ctx);
VGX_API int vgx_ctx_synchronize_tsdf(vgx_ctx ctx);
VGX_API int vgx_ctx_tsdf_wait_for_stream(vgx_ctx ctx, void* producer_stream);
VGX_API int vgx_ctx_stream_priorities(vgx_ctx ctx);
/* How the sampling grids of the submaps created on this context FROM NOW ON are laid out in HBM (set it
 * once, before the first submap; a batch refuses to mix layouts).  Results never depend on it.
 *   VGX_BRICKS_APRON (default)  17^3 floats per block; fewest bytes: fastest where every registration
 *                               point is evaluated (sampling_ratio -1).
 *   VGX_BRICKS_QUAD             a 2x2x2 neighbourhood is 32 contiguous bytes (4.25 x the memory):
 *                               fastest where evaluations are scattered -- the reference's shipped
 *                               sampling_ratio 0.05 (voxgraph_mapper.yaml:34): -14 % per solver evaluation,
 *                               at +18-25 % on the all-points passes. */
#define VGX_BRICKS_APRON 0
#define VGX_BRICKS_QUAD 1
VGX_API int vgx_ctx_set_brick_layout(vgx_ctx ctx, int32_t layout);
/* Sampling sessions (round 4).  A vgx_reg_batch whose constraints ALL sample (sampling_ratio != -1: the
 * reference's shipped 0.05, voxgraph_mapper.yaml:34) evaluates scattered points, where every 128-byte line a
 * neighbourhood touches is an HBM fetch of its own; on a context whose submaps hold apron bricks such a batch
 * therefore reads QUAD bricks, made on demand from the apron bricks of the submaps it reads (a device-side
 * copy at batch creation, kept with the submap: + 4.25 x the grid memory of those submaps only) -- the
 * all-points passes of the same context keep their apron bricks.  Results never depend on it.
 *   VGX_SAMPLING_BRICKS_QUAD (default)   as described
 *   VGX_SAMPLING_BRICKS_SAME             sampling batches read the bricks everything else reads */
#define VGX_SAMPLING_BRICKS_SAME 0
#define VGX_SAMPLING_BRICKS_QUAD 1
VGX_API int vgx_ctx_set_sampling_bricks(vgx_ctx ctx, int32_t mode);
/* which bricks a batch reads (VGX_BRICKS_APRON / VGX_BRICKS_QUAD); -1 for a NULL handle */
VGX_API int32_t vgx_reg_batch_brick_layout(vgx_reg_batch batch);
VGX_API int vgx_ctx_synchronize(vgx_ctx ctx);
/* hipEvent-based timer on the context's stream (used by bench.py so that
 * the kernel time is measured on the stream the kernels run on). */
VGX_API int vgx_ctx_timer_start(vgx_ctx ctx);
VGX_API int vgx_ctx_timer_stop(vgx_ctx ctx, float* elapsed_ms);

/* ---- submaps ----------------------------------------------------------- */
/* Stands in for a *finished* voxgraph::VoxgraphSubmap
 * (include/voxgraph/frontend/submap_collection/voxgraph_submap.h:16): the
 * TSDF and ESDF voxblox layers (same voxel size and voxels_per_side,
 * voxgraph_submap.cpp:26-29) plus its cached registration points.  A submap
 * is immutable once uploaded -- the invariant the reference relies on to
 * optimise while integrating (voxgraph_mapper.cpp:464-471).
 *
 * Layer layout = voxblox's: block b covers block_index[b] * (vps*voxel_size);
 * per-block arrays hold vps^3 voxels, linear index x + vps*(y + vps*z).
 * Any of the four voxel arrays may be NULL when that layer is not needed
 * (REG with use_esdf_distance reads only esdf_*; point extraction reads
 * tsdf_* and, with use_esdf_distance, esdf_distance).
 * Distances of valid voxels must be finite. */
VGX_API int vgx_submap_create(vgx_ctx ctx, int32_t submap_id, float voxel_size,
                              int32_t voxels_per_side, int32_t n_blocks,
                              const int32_t* block_index /* [n_blocks][3] */,
                              const float* tsdf_distance /* [n_blocks][vps^3] */,
                              const float* tsdf_weight,
                              const float* esdf_distance,
                              const uint8_t* esdf_observed,
                              vgx_submap* out);
/* Lifetimes follow the reference's ownership: a RegistrationCostFunction holds VoxgraphSubmap::ConstPtr to both submaps
 * (registration_cost_function.h), a ceres::Problem owns its cost functions.  So destroying a submap that cost functions
 * were built on is DEFERRED to the destruction of the last of them (the call returns VGX_OK at once and the handle must
 * not be used again by the caller); likewise vgx_reg_destroy on a cost function that batches still list is carried out
 * by the last vgx_reg_batch_destroy.  Contexts are not counted: destroy a context last. */
VGX_API int vgx_submap_destroy(vgx_submap submap);
VGX_API int32_t vgx_submap_id(vgx_submap submap);
VGX_API int32_t vgx_submap_num_blocks(vgx_submap submap);

/* VoxgraphSubmap::RegistrationPointType (voxgraph_submap.h:65) */
#define VGX_POINTS_ISOSURFACE 0
#define VGX_POINTS_VOXELS 1

/* vgx_submap_set_points flags */
#define VGX_POINTS_KEEP_ORDER 0u
/* Re-order the points along a Morton curve of their voxel coordinates so a
 * wavefront's 64 points gather from neighbouring cache lines.  Residual i
 * then refers to uploaded point order[i] (vgx_submap_point_order); Ceres is
 * indifferent to residual order, and every residual row still pairs with its
 * own Jacobian row. */
#define VGX_POINTS_SORT_MORTON 1u

/* Upload cached registration points (RegistrationPoint,
 * registration_point.h:6-12): position in the submap frame, distance, weight. */
VGX_API int vgx_submap_set_points(vgx_submap submap, int32_t point_type,
                                  int64_t n, const float* xyz /* [n][3] */,
                                  const float* distance, const float* weight,
                                  uint32_t flags);
/* Device-side VoxgraphSubmap::findRelevantVoxelIndices
 * (voxgraph_submap.cpp:144-201): stream-compacts every TSDF voxel with
 * weight > min_voxel_weight && |distance| < max_voxel_distance into the
 * VGX_POINTS_VOXELS set, in block order then (by default) linear-index order.
 * Needs tsdf_* (and esdf_distance if use_esdf_distance). */
VGX_API int vgx_submap_extract_voxel_points(vgx_submap submap,
                                            double min_voxel_weight,
                                            double max_voxel_distance,
                                            int32_t use_esdf_distance,
                                            int64_t* n_points_out);
/* Device-side VoxgraphSubmap::findIsosurfaceVertices (voxgraph_submap.cpp:203-243), the
 * VGX_POINTS_ISOSURFACE set the shipped "explicit_to_implicit" method registers with:
 * zero crossings of the TSDF along the edges of every fully observed dual cell (all 8
 * corner voxels with weight > min_weight: voxblox MeshIntegrator), merged per
 * 0.5-voxel cell (MeshLayer::getConnectedMesh(mesh, 0.5 * voxel_size)), each carrying the
 * trilinearly interpolated TSDF distance and weight (Interpolator::getVoxel).  Which of
 * several vertices in one cell survives is implementation-defined in the reference
 * (unordered_map order); here it is the first in (block, linear index, axis) order.
 * Needs the raw TSDF layer.  Also records the blocks that contain vertices
 * (isosurface_blocks_, voxgraph_submap.cpp:237-240). */
VGX_API int vgx_submap_extract_isosurface_points(vgx_submap submap, double min_voxel_weight,
                                                 int64_t* n_points_out);
VGX_API int64_t vgx_submap_num_points(vgx_submap submap, int32_t point_type);
/* order[i] = index (in upload / extraction order) of the point residual i uses */
VGX_API int vgx_submap_point_order(vgx_submap submap, int32_t point_type,
                                   int64_t* order /* [n] */);
/* Copy the (re-ordered) device point set back: xyz[n][3], distance, weight. */
VGX_API int vgx_submap_download_points(vgx_submap submap, int32_t point_type,
                                       float* xyz, float* distance,
                                       float* weight);
/* Copy the raw voxel layers back ([n_blocks][vps^3] each, any pointer may be
 * NULL) and the block index list ([n_blocks][3]). */
VGX_API int vgx_submap_download_layers(vgx_submap submap, float* tsdf_distance,
                                       float* tsdf_weight, float* esdf_distance,
                                       uint8_t* esdf_observed);
VGX_API int vgx_submap_block_index(vgx_submap submap, int32_t* block_index);
/* Device-side cblox::TsdfEsdfSubmap::generateEsdf() (voxgraph_submap.cpp:86), i.e.
 * voxblox::EsdfIntegrator::updateFromTsdfLayerBatch [recalled]: TSDF voxels with
 * weight >= min_weight become observed; |tsdf| < min_distance_m is copied and fixed;
 * the rest starts at sign * default_distance_m and is lowered by the quasi-Euclidean
 * 26-neighbour wavefront (steps 1, sqrt2, sqrt3 voxels) from voxels closer than
 * max_distance_m, never across a sign change.  voxblox runs a bucketed label-correcting
 * queue that ignores improvements below min_diff_m (1 mm); the GPU relaxes to the exact
 * fixed point of the same recurrence, so results agree to within a few min_diff_m
 * (min_diff_m and num_buckets are accepted for layout compatibility and ignored): worst 2.54 mm over 174.7 M fuzzed voxels.  One
 * discontinuity, outside voxblox's defaults only: when default_distance_m > max_distance_m, a voxel of the shell beyond the limit
 * whose neighbour sits within that slack of it can take another neighbour's longer path or keep the default.
 * Fills the ESDF raw layer from the resident TSDF layer and rebuilds the ESDF sampling
 * grid.  cfg == NULL uses voxblox's defaults.  sweeps (nullable) = global passes used.
 * The result's bits are determined: it is the greatest fixed point of the f32 recurrence, whatever order the blocks ran in
 * (tests/esdf_ref.py restates it in numpy, and the tests compare bit for bit).
 * Configuration: max_distance_m > 0, default_distance_m > 0 and min_distance_m >= 0 are required (a NaN fails each), nothing
 * else.  max_distance_m and default_distance_m may be huge or +inf (an uncapped ESDF): the number of passes is limited by
 * 8 + 2 * ceil(max_distance_m / voxel_size) AND by the submap's voxel count + 1 (a best path visits no voxel twice), formed in
 * floating point, so every valid configuration runs to the fixed point.  Should the limit ever be reached with voxels still
 * changing, the call returns VGX_ERR_INVALID with a message, never VGX_OK over a partly relaxed layer; the ESDF sampling grid
 * is then absent (it is dropped as soon as the layer is rewritten, also when a HIP call fails).
 * Edges, as they are (the restated queue, oracle/esdf_oracle.c, does the same on each; none is changed quietly here):
 *  - min_distance_m = 0 fixes no voxel, so nothing is a surface voxel and every observed voxel keeps sign * default_distance_m:
 *    a layer without a single distance in it.  min_distance_m above the TSDF's truncation distance likewise fixes every voxel
 *    the TSDF clipped, at the truncation distance.
 *  - a TSDF distance of exactly +-0 outside the band (possible only with min_distance_m = 0) and a NaN TSDF distance under a
 *    weight >= min_weight both have no sign: the voxel becomes observed with distance +0, is never a source and is never
 *    updated -- an observed "surface" voxel that nobody measured.  With default_distance_m = inf it is 0 * inf = NaN instead.
 *  - a NaN weight is not < min_weight, so the voxel counts as observed.
 *  - max_distance_m below one voxel step: only fixed voxels below it are sources, their neighbours get one step, nothing
 *    further moves; with default_distance_m <= one step nothing moves at all.
 *  - default_distance_m < max_distance_m: voxels still at the default are sources too, harmlessly (default + step never
 *    improves on the default); values above the default are never written. */
typedef struct vgx_esdf_config {
  float max_distance_m;     /* 2.0   */
  float min_distance_m;     /* 0.2   */
  float default_distance_m; /* 2.0   */
  float min_diff_m;         /* 0.001 (ignored) */
  float min_weight;         /* 1e-6  */
  int32_t num_buckets;      /* 20    (ignored) */
} vgx_esdf_config;
VGX_API void vgx_esdf_config_default(vgx_esdf_config* cfg);
VGX_API int vgx_submap_generate_esdf(vgx_submap submap, const vgx_esdf_config* cfg,
                                     int32_t* sweeps);
/* Drop the raw voxel layers after extraction (keeps the sampling grids). */
VGX_API int vgx_submap_release_raw_layers(vgx_submap submap);

/* ---- REG: one registration constraint ---------------------------------- */
/* RegistrationCostFunction::Config (registration_cost_function.h:17-41).
 * jacobian_evaluation_method is always analytic.  visualize_residuals / visualize_gradients are the two want_* arguments
 * of vgx_reg_evaluate_visuals ("Cost-function visuals" below); visualize_transforms_ needs no device: the C++ adapter
 * hands T_mission__reading to its sink (voxgraph_amd/cpp/gpu_cost_function_visuals.h). */
typedef struct vgx_reg_config {
  int32_t registration_point_type; /* VGX_POINTS_*, default ISOSURFACE (h:20) */
  float sampling_ratio;            /* -1 disables sampling (h:28)             */
  double no_correspondence_cost;   /* default 0 (h:32)                        */
  int32_t use_esdf_distance;       /* default 1 (h:35)                        */
  uint32_t sampler_seed;           /* 0 (default): draw from the reference submap's own
                                    * sampler stream -- one default-seeded (5489)
                                    * std::mt19937 per point set, advanced by every cost
                                    * function sampling that set, as WeightedSampler does
                                    * (weighted_sampler.h:36-39).  != 0: a private engine
                                    * seeded with this value                              */
} vgx_reg_config;
VGX_API void vgx_reg_config_default(vgx_reg_config* cfg);

/* new RegistrationCostFunction(reference_submap, reading_submap, config)
 * (registration_cost_function.cpp:12-56; construction sites
 * registration_constraint.cpp:33-35, submap_registration_helper.cpp:44-46,
 * map_evaluation.cpp:143-144).  Cheap: no device allocation proportional to
 * the point count happens until the first evaluate. */
VGX_API int vgx_reg_create(vgx_ctx ctx, vgx_submap reference_submap,
                           vgx_submap reading_submap, const vgx_reg_config* cfg,
                           vgx_reg* out);
VGX_API int vgx_reg_destroy(vgx_reg reg);
/* num_residuals() (registration_cost_function.cpp:45-55) */
VGX_API int64_t vgx_reg_num_residuals(vgx_reg reg);

/* Drop-in for ceres::CostFunction::Evaluate
 * (registration_cost_function.h:47-48, .cpp:58-298):
 *   parameters[0] = ref_pose  {x,y,z,yaw} of the reference (first) submap,
 *   parameters[1] = read_pose {x,y,z,yaw} of the reading (second) submap,
 *   residuals[N]; jac_ref / jac_read are jacobians[0] / jacobians[1], each
 *   [N][4] row-major f64, either or both may be NULL.
 * All outputs are already scaled by N / sum(w) (.cpp:274-291).
 * Returns VGX_OK (true), VGX_EVALUATE_FALSE (false) or an error. */
VGX_API int vgx_reg_evaluate(vgx_reg reg, const double ref_pose[4],
                             const double read_pose[4], double* residuals,
                             double* jac_ref, double* jac_read);

/* Same evaluation, results left on the device as f32 (the 88 B/evaluation
 * form): DEVICE pointers residuals[N], jac_ref[N][4], jac_read[N][4]
 * (16-byte aligned), either Jacobian may be NULL. Asynchronous on the
 * context's stream. */
VGX_API int vgx_reg_evaluate_device_f32(vgx_reg reg, const double ref_pose[4],
                                        const double read_pose[4],
                                        void* d_residuals, void* d_jac_ref,
                                        void* d_jac_read);

/* ---- REG: cost-function visuals ------------------------------------------ */
/* Cost-function visuals: what RegistrationCostFunction::Evaluate hands to CostFunctionVisuals while it evaluates
 * (registration_cost_function.cpp:169-176, 244-252, 293-295, cited as RCF; cost_function_visuals.cpp:43-101, CFV) -- the
 * residual cloud (pcl::PointCloud<pcl::PointXYZI>, topic cost_residuals) and the two Jacobian markers (cost_jacobians)
 * that registration_test_bench shows while a registration converges.  vgx_reg_evaluate_visuals is vgx_reg_evaluate plus
 * the visuals of that same evaluation, left in a reusable handle.
 * Rules (what the kernel, vgx_reg.hip, and the restatement, tests/cost_visuals_ref.py, both follow):
 *   rows        row i runs over the registration points, or in sampling mode over this evaluation's draws in draw
 *               order with weight 1 (RCF:113-122); n = num_residuals.
 *   p_read      T_reading__reference * p_ref in f32: the point the residual is interpolated at.
 *   p_m         T_mission__reading * p_read in f32, minkindr's point transform (v + w uv + u x uv with uv = 2 u x v,
 *               then + t), T_mission__reading = exp of the reading pose narrowed to f32 (RCF:80-88).
 *   r_u, j      the UNSCALED f64 residual (RCF:161-166; w * no_correspondence_cost without a correspondence) and the
 *               unscaled f32 pResidual_pParamRead.head<3>() (RCF:249; zero without a correspondence).
 *   factor      num_residuals / summed_weight (RCF:274); 1 in sampling mode.
 *   cloud       one 32-byte pcl::PointXYZI record per row, in row order, the layout of vgx_submap_surface_msg: x y z
 *               f32 of p_m at bytes 0, 4, 8, 1.0f at byte 12, intensity at byte 16, bytes 20..31 zero.
 *               intensity = (float)((double)(float)r_u * factor): CFV:49 narrows, CFV:75 multiplies a float by a double
 *               in f64 and rounds once.
 *   gradients   filled iff want_gradients and at least one of jac_ref / jac_read is given (RCF:179: jacobians !=
 *               nullptr).  o = (double)p_m; t = (double)j * (factor * 0.05) + o, in f64: the product factor * 0.05
 *               first, then one multiply, then one add, never contracted (CFV:82-89).
 *               arrow_points [2n][3] f64 = o0 t0 o1 t1 .. (the LINE_LIST marker), origin_points [n][3] f64 = o0 o1 ..
 *               (the SPHERE_LIST marker).  The fixed marker fields (CFV:13-40) are host constants of the C++ adapter.
 *   false       when the summed weight is 0 Evaluate returns false before anything is published (RCF:273): VGX_EVALUATE_
 *               FALSE, and the handle holds 0 points.  The reference does NOT reset its accumulators on that path, so
 *               its next publication carries the stale points too; that is its bug and is not reproduced.
 * residuals / jac_ref / jac_read are bit for bit what vgx_reg_evaluate returns at the same poses; in sampling mode the
 * call consumes exactly one evaluation's engine outputs and the visuals show that evaluation's draws.  One more kernel
 * on the evaluation slot's stream (no dead-tile shortcut: a tile outside the reading grid still has positions and the
 * no-correspondence intensity), no host synchronisation beyond vgx_reg_evaluate's own.  Per row the kernel writes 32 B
 * (cloud) + 48 B + 24 B (gradients) in 16-byte stores.
 * Refused with VGX_ERR_INVALID before anything is launched: a NULL visuals handle, one of another context (the handle
 * keeps what it held), residuals == NULL, registration points replaced since the cost function was created.  The handle
 * is reused from call to call: its device buffers grow on demand; one call at a time per handle.  want_residual_cloud
 * == 0: 0 cloud points.  Out of scope: the batched entry points, ROS / PCL types, the box, pose-history and pose-graph-
 * edge markers. */
typedef struct vgx_reg_visuals_s* vgx_reg_visuals;
VGX_API int vgx_reg_visuals_create(vgx_ctx ctx, vgx_reg_visuals* out);
VGX_API int vgx_reg_visuals_destroy(vgx_reg_visuals visuals);
VGX_API int vgx_reg_evaluate_visuals(vgx_reg reg, const double ref_pose[4], const double read_pose[4],
                                     double* residuals, double* jac_ref, double* jac_read,
                                     int32_t want_residual_cloud, int32_t want_gradients, vgx_reg_visuals visuals);
/* of the last evaluation into the handle; n_jacobians is 0 when no Jacobians were asked for; either may be NULL */
VGX_API int vgx_reg_visuals_stats(vgx_reg_visuals visuals, int64_t* n_residual_points, int64_t* n_jacobians);
/* cloud_bytes [32 n_residual_points], arrow_points [2 n_jacobians][3] f64, origin_points [n_jacobians][3] f64, the
 * factor of that evaluation (0 when the handle holds nothing); any argument may be NULL */
VGX_API int vgx_reg_visuals_download(vgx_reg_visuals visuals, void* cloud_bytes, double* arrow_points,
                                     double* origin_points, double* factor);
/* the device arrays held now (NULL for an array with 0 rows); valid until the next evaluation into the handle or destroy */
VGX_API int vgx_reg_visuals_device_pointers(vgx_reg_visuals visuals, const void** cloud, const double** arrow_points,
                                            const double** origin_points);

/* ---- REG: all constraints of a pose graph in one launch ----------------- */
/* Mirrors one pass of the Ceres evaluator over every registration residual
 * block (pose_graph.cpp:101): constraint c links node_pair[c][0] (reference,
 * first submap) to node_pair[c][1] (reading, second submap).
 * global_index (nullable) gives each constraint's index in the whole graph
 * when the constraint list is sharded across processes; n_global is the
 * unsharded constraint count (values below n are read as n when global_index == NULL; a
 * shard that owns no constraint at all passes n = 0, global_index = NULL and the real n_global,
 * so that its assembled buffer has -- and zeroes -- the full size). */
VGX_API int vgx_reg_batch_create(vgx_ctx ctx, int32_t n, const vgx_reg* regs,
                                 const int32_t* node_pair /* [n][2] */,
                                 const int32_t* global_index /* [n] or NULL */,
                                 int32_t n_global, vgx_reg_batch* out);
VGX_API int vgx_reg_batch_destroy(vgx_reg_batch batch);
VGX_API int64_t vgx_reg_batch_num_residuals(vgx_reg_batch batch);
/* row_offset[c] = first row of constraint c in the stacked outputs; [n+1] */
VGX_API int vgx_reg_batch_row_offsets(vgx_reg_batch batch, int64_t* row_offset);

/* Materialising pass: residual + both Jacobians of every constraint as f32
 * into DEVICE arrays stacked by row_offset: residuals[R], jac_ref[R][4],
 * jac_read[R][4].  poses: host [n_nodes][4] f64.  status[c] (host, nullable)
 * receives VGX_OK / VGX_EVALUATE_FALSE per constraint.  Asynchronous.
 * Alignment: 16 bytes is required (float4 stores); more buys nothing (measured
 * with the placement held fixed: profiles/r05_points_placement.txt).  WHERE the
 * arrays lie physically does matter: vgx_reg_batch_choose_outputs below.
 * Each wavefront stores whole 64-row spans counted from the arrays' bases, whatever a constraint's row_offset is (a batch
 * launched in the grouped order keeps its point loads aligned instead); that saves the split sectors only on bases aligned
 * to 256 bytes, as hipMalloc's and torch's are (profiles/points_row_alignment.txt). */
VGX_API int vgx_reg_batch_evaluate_points(vgx_reg_batch batch,
                                          const double* poses, int32_t n_nodes,
                                          void* d_residuals, void* d_jac_ref,
                                          void* d_jac_read, int32_t* status);

/* The same pass in Ceres' own types: residuals[R] and jac_*[R][4] as F64, every value the f64 the reference's Evaluate writes
 * (registration_cost_function.cpp:163-166, 254-267, scaled as :274-291) -- what vgx_reg_evaluate returns for one constraint,
 * for the whole list in one launch and left on the device (72 B per row written instead of 36: SURVEY.md 8d's "124 B"
 * variant).  Same arguments and status as vgx_reg_batch_evaluate_points; jac_* 32-byte aligned (one row). */
VGX_API int vgx_reg_batch_evaluate_points_f64(vgx_reg_batch batch, const double* poses /* [n_nodes][4] */, int32_t n_nodes,
                                              void* d_residuals, void* d_jac_ref, void* d_jac_read, int32_t* status);

/* The same rows KEPT BY THE BATCH, and one constraint's slice of them fetched to the host -- SURVEY.md 8b's "vgx_reg_fetch(h,
 * residuals, jac_ref, jac_read) for the cached per-constraint slice": ONE launch per solver evaluation, and every residual block
 * still the reference's own N-residual block (f64, Ceres layout, every value the reference's: a ceres::LossFunction or a
 * covariance estimate sees exactly what RegistrationCostFunction::Evaluate would have given it), where the drop-in
 * vgx_reg_evaluate is one launch per block.  evaluate_rows_f64: want_jac_* = 0 leaves that block's Jacobians out (Ceres passes
 * jacobians == NULL, or the block is constant); the arrays are the batch's own (72 B per row, allocated at first use, with a
 * pinned host mirror filled by one copy per evaluation while they are below 2 GiB).  fetch_rows_f64(c, ...): any output may
 * be NULL; waits for the evaluation; VGX_ERR_INVALID without one, or for a Jacobian block it was not asked for.
 * voxgraph_amd/cpp/gpu_registration_rows.h is the ceres::EvaluationCallback built on the pair. */
VGX_API int vgx_reg_batch_evaluate_rows_f64(vgx_reg_batch batch, const double* poses /* [n_nodes][4] */, int32_t n_nodes,
                                            int32_t want_jac_ref, int32_t want_jac_read, int32_t* status);
VGX_API int vgx_reg_batch_fetch_rows_f64(vgx_reg_batch batch, int32_t constraint, double* residuals, double* jac_ref,
                                         double* jac_read);


/* The same pass into ONE output stream: an array of tile blocks, one block per rows_per_block (1024) consecutive residuals
 * of a constraint -- block = [residual f32 x 1024][jac_ref f32x4 x 1024][jac_read f32x4 x 1024], 36 KiB, every constraint
 * padded to whole blocks (its last block's unused rows are not written).  Residual k of constraint c is row k % 1024 of
 * block first_block[c] + k / 1024.  For consumers that live on the device and do not need three Ceres-shaped arrays: one
 * write front instead of three (profiles/r05_points_placement.txt says what three cost on an unlucky placement).
 * vgx_reg_batch_blocked_layout: bytes = size of the array; first_block (nullable) = [n + 1]. */
VGX_API int vgx_reg_batch_blocked_layout(vgx_reg_batch batch, int64_t* bytes, int32_t* rows_per_block,
                                         int64_t* first_block);
VGX_API int vgx_reg_batch_evaluate_points_blocked(vgx_reg_batch batch, const double* poses, int32_t n_nodes,
                                                  void* d_blocks, int32_t* status);

/* Placement by measurement.  WHERE the output arrays of the materialising pass lie in physical memory decides which of
 * two speeds the kernel runs at -- 200 x 256^3 submaps, 1176 constraints: 4.4-4.7 ms or 5.3-5.7 ms per launch; about half
 * of the sets of three an allocator hands out are slow ones, a matter of how the arrays lie relative to each other: every
 * array's own fill and read rate is the same (measured: profiles/r05_points_placement.txt).  The physical address is not the caller's to choose, but which of several
 * allocations to keep is: given n_candidates device pointers for each array (each large enough for the batch; d_jac_ref /
 * d_jac_read may be NULL as for the pass itself), this call times the batch's own launch -- one warm-up and `launches`
 * timed launches per trial -- first on whole sets (the k-th candidate of each array), then array by array against the
 * best combination so far, and returns in chosen[] the index to keep for residuals, jac_ref and jac_read.  ms_chosen
 * (nullable): ms per launch of that combination.  ms_trials (nullable, [n_candidates * 4]): every trial in order -- the n
 * sets, then jac_read's, jac_ref's and the residuals' candidates (-1 where a candidate needed no new trial).  The arrays
 * are overwritten.  Synchronous.  4 candidates and 3 launches cost 13 trials of 4 launches.
 * REFUSED (VGX_ERR_INVALID) for a batch with sampling constraints: every trial is launches + 1 evaluations of the batch,
 * and an evaluation of a sampling batch DRAWS -- it would leave every reference point set's std::mt19937 dozens of
 * evaluations further on and break "one evaluation of the batch = one Evaluate of every constraint in list order".  Where
 * the arrays lie does not depend on which points are drawn: choose with an all-points batch of the same sizes. */
VGX_API int vgx_reg_batch_choose_outputs(vgx_reg_batch batch, const double* poses, int32_t n_nodes,
                                         int32_t n_candidates, void* const* d_residuals, void* const* d_jac_ref,
                                         void* const* d_jac_read, int32_t launches, int32_t chosen[3],
                                         float* ms_chosen, float* ms_trials);

/* The same, with the arrays the library's own: allocates n_candidates (1..16) sets of the row arrays the batch needs (f32:
 * residuals [R], jac_* [R][4]; want_jac_* = 0 leaves that array out), chooses among them as vgx_reg_batch_choose_outputs does
 * (3 launches per trial), frees the unchosen ones and returns the three pointers to keep -- one call instead of "allocate a
 * few, choose, free the rest"; transient memory n_candidates x 36 B x R (fewer sets are tried when the device runs out).  A
 * sampling batch gets the first set untimed (its trial evaluations would advance the engines).  ms_chosen (nullable): ms per
 * launch on the arrays returned (0 when nothing was timed).  Release them with vgx_reg_batch_free_outputs while the batch
 * lives (it waits for the batch's stream first). */
VGX_API int vgx_reg_batch_alloc_outputs(vgx_reg_batch batch, const double* poses, int32_t n_nodes, int32_t n_candidates,
                                        int32_t want_jac_ref, int32_t want_jac_read, void** d_residuals, void** d_jac_ref,
                                        void** d_jac_read, float* ms_chosen);
VGX_API int vgx_reg_batch_free_outputs(vgx_reg_batch batch, void* d_residuals, void* d_jac_ref, void* d_jac_read);

/* Fused pass: no per-point outputs.  Per constraint c, 45 f64:
 *   [0]      sum r^2
 *   [1..8]   J^T r      over the stacked parameters [ref(4), read(4)]
 *   [9..44]  upper triangle of J^T J (row-major, 8x8)
 * d_normal: DEVICE pointer [n][45] (nullable); normal_host: host [n][45]
 * (nullable; implies a stream synchronisation).
 * Deterministic: fixed reduction tree, no atomics. */
VGX_API int vgx_reg_batch_evaluate_normal(vgx_reg_batch batch,
                                          const double* poses, int32_t n_nodes,
                                          void* d_normal, double* normal_host,
                                          int32_t* status);

/* Fused pass, COST ONLY: per constraint c one f64, sum r^2 -- element [0] of vgx_reg_batch_evaluate_normal's block at the
 * same poses, BIT FOR BIT (the same f32 operations in the same order, the same reduction tree; all-points batches -- a
 * sampling batch draws anew, see below).  The reference does no Jacobian work when Ceres passes `jacobians == nullptr`
 * (registration_cost_function.cpp:179), and Ceres' Levenberg-Marquardt evaluates every TRIAL step that way
 * (pose_graph.cpp:90-101): this is that evaluation for the whole constraint list -- no gradient, no pose-Jacobian
 * products, one running sum per lane instead of 21, nothing to compress afterwards.
 * d_cost: DEVICE pointer [n] f64 (nullable); cost_host: host [n] (nullable; implies a stream synchronisation).
 * With d_cost == NULL the batch's internal block array serves as scratch: the blocks a previous
 * vgx_reg_batch_evaluate_normal(d_normal == NULL) left there (what vgx_reg_batch_assemble / _scatter_normal read when
 * THEY are given NULL) are gone -- evaluate the blocks again before assembling.  The batch keeps count of it:
 * vgx_reg_batch_assemble / _scatter_normal with d_normal == NULL return VGX_ERR_INVALID ("the batch's internal array holds
 * no blocks") until a vgx_reg_batch_evaluate_normal(d_normal == NULL) has succeeded on the handle with no cost-only
 * evaluation into the internal array since.  An evaluation into the caller's own arrays leaves the internal blocks, and
 * whether they can be read, as they were.  Deterministic.
 * SAMPLING constraints (sampling_ratio != -1): EVERY evaluation of a batch -- points, normal or cost -- is one Evaluate of
 * every constraint in list order and DRAWS its points from the reference point sets' engines, as every call of the
 * reference's Evaluate does (registration_cost_function.cpp:113-122): a cost-only evaluation followed by a full one at the
 * same poses sees two different draws, exactly like Ceres on the reference.  A caller that serves a second request at
 * an unchanged point from what it cached (the C++ adapters, when Ceres says new_evaluation_point == false and what it
 * asks for is cached) does NOT redraw where the reference would: fewer draws, each still a legal one. */
VGX_API int vgx_reg_batch_evaluate_cost(vgx_reg_batch batch, const double* poses, int32_t n_nodes, void* d_cost,
                                        double* cost_host, int32_t* status);

/* Measurement aid for the fused pass: the number of residuals whose registration points the
 * fused kernel actually reads at these poses, i.e. the points of every 512-point chunk whose
 * bounding sphere can touch the reading submap's block box (chunks that cannot are skipped
 * without loading their points when no_correspondence_cost == 0); and (nullable) the number of
 * DISTINCT points behind them -- constraints that share a reference submap read the same points,
 * which the fused pass's launch order lets them share through one XCD's L2.  Synchronous. */
VGX_API int vgx_reg_batch_count_live(vgx_reg_batch batch, const double* poses, int32_t n_nodes,
                                     int64_t* live_residuals, int64_t* unique_points);

/* The same count per constraint (live_each[n], batch order): what a constraint costs at these poses is
 * roughly 36 B x its residuals + 45 B x its live residuals, which is a better weight for
 * vgx_lpt_shards than the residual count alone when much of the constraint list is culled. */
VGX_API int vgx_reg_batch_count_live_each(vgx_reg_batch batch, const double* poses, int32_t n_nodes,
                                          int64_t* live_each);

/* Measurement aid: which launch order the batch's tiles took at their first evaluation.  pass 0 =
 * fused (evaluate_normal), 1 = materialising (evaluate_points).  *grouped = 1: constraints that share
 * a reference submap run side by side on one XCD and read its points through that XCD's L2 once;
 * 0: plain constraint-major order (nothing worth sharing, or too much culled); -1: that pass has not
 * run yet.  Results never depend on the order. */
VGX_API int vgx_reg_batch_launch_order(vgx_reg_batch batch, int32_t pass, int32_t* grouped);

/* Scatter-adds this process's [n][45] blocks into the fused buffer every
 * process all-reduces once per solver evaluation, DEVICE f64:
 *   [0]                               sum of costs
 *   [1 .. 4*n_nodes]                  J^T r per node
 *   [.. + 16*n_nodes]                 diagonal 4x4 blocks of J^T J per node
 *   [.. + 16*n_global]                off-diagonal 4x4 block (ref rows, read
 *                                     cols) per constraint, written by exactly
 *                                     one process
 * The buffer is zeroed first when `zero_first` != 0. */
VGX_API int vgx_reg_batch_assemble(vgx_reg_batch batch, const void* d_normal,
                                   int32_t n_nodes, void* d_fused,
                                   int32_t zero_first);
VGX_API int64_t vgx_reg_fused_size(int32_t n_nodes, int32_t n_global);

/* Sharding-independent assembly (round 4).  vgx_reg_batch_assemble sums a node's entries over the shard's
 * own constraints, so a sum of per-shard fused buffers depends, in its last bits, on how the list was
 * sharded and on the order a collective adds in.  Exchanging the per-constraint BLOCKS instead makes the
 * result the single-GPU one bit for bit, for any number of shards:
 *   1. every shard:  vgx_reg_batch_evaluate_normal, then vgx_reg_batch_scatter_normal writes its [n][45]
 *      blocks (d_normal NULL: the batch's own) into rows global_index[c] of a DEVICE [n_global][45] f64
 *      array, zeroed first when zero_first != 0;
 *   2. ONE all-reduce(sum) of that array (n_global x 360 B: 423 KB for 1176 constraints), its words taken as
 *      64-bit INTEGERS: every row is written by exactly one shard and is all-zero-bits everywhere else, so
 *      the integer sum is that shard's bit pattern in ANY order (an f64 sum is exact too, but turns a -0.0
 *      into +0.0);
 *   3. vgx_reg_assembler_assemble builds the fused buffer (layout above, vgx_reg_fused_size(n_nodes, n))
 *      from the complete array in list order -- what a single vgx_reg_batch over the whole list computes.
 * The assembler holds the list's node structure (node_pair[n][2], the caller's constraint order) on `ctx`. */
VGX_API int vgx_reg_batch_scatter_normal(vgx_reg_batch batch, const void* d_normal, void* d_normal_all,
                                         int32_t zero_first);
VGX_API int vgx_reg_assembler_create(vgx_ctx ctx, int32_t n, const int32_t* node_pair /* [n][2] */,
                                     vgx_reg_assembler* out);
VGX_API int vgx_reg_assembler_assemble(vgx_reg_assembler assembler, const void* d_normal_all, int32_t n_nodes,
                                       void* d_fused);
VGX_API int vgx_reg_assembler_destroy(vgx_reg_assembler assembler);

/* Host-side helper for solvers that want residual blocks (Ceres), not normal equations:
 * turns one constraint's 45-number block N = [J r]^T [J r] into a 9-residual block with
 * the same normal equations, r_c[9] and J_c[9][8] row-major (J_c^T J_c = J^T J,
 * J_c^T r_c = J^T r, r_c^T r_c = r^T r), via a symmetric eigen-decomposition
 * N = V L V^T, [J_c | r_c] = sqrt(max(L, 0)) V^T.  Exact for least squares without a robust
 * loss, which is how the reference adds registration constraints
 * (registration_constraint.cpp:10, constraint.h:34).  Pure host arithmetic. */
VGX_API int vgx_reg_compress_normal(const double normal[45], double residuals9[9],
                                    double jacobian9x8[72]);

/* ---- REG on several GPUs of one process --------------------------------- */
/* voxgraph is one process (voxgraph_mapping_node.cpp:6-26); given the poses its registration
 * constraints are independent, so the list is pair-sharded over N contexts -- one per
 * GPU, every finished submap uploaded to each -- and each solver evaluation ends in ONE reduction.
 *
 * vgx_lpt_shards: greedy longest-processing-time partition; weight[c] = the constraint's residual
 * count (keep both directions of a mirrored pair together by giving them one entry).  Create each
 * constraint's cost function on the context of its shard, then hand the whole list over:
 * vgx_reg_multi_create sorts the constraints by owning context, builds one vgx_reg_batch per
 * context and starts one host thread per context.  Contexts may share a device (testing). */
VGX_API int vgx_lpt_shards(int32_t n, const int64_t* weight, int32_t n_shards, int32_t* shard_of /* [n] */);
/* The locality-aware alternative: the list cut into n_shards CONSECUTIVE runs of (nearly) equal weight
 * (constraint c goes to the shard its weight midpoint falls in).  voxgraph creates constraints in submap
 * order, i.e. along the trajectory, so a shard then touches the submaps of one stretch of the map and only
 * those need to be resident on its GPU -- a third of the map instead of three quarters at N = 8 on the bench
 * graphs, for a balance a few per cent behind LPT's (profiles/r04_shard_balance.json).
 * Results never depend on the placement (see "Sharding-independent assembly"). */
VGX_API int vgx_contiguous_shards(int32_t n, const int64_t* weight, int32_t n_shards, int32_t* shard_of /* [n] */);
VGX_API int vgx_reg_multi_create(int32_t n_ctx, const vgx_ctx* ctxs, int32_t n, const vgx_reg* regs,
                                 const int32_t* node_pair /* [n][2] */, vgx_reg_multi* out);
VGX_API int vgx_reg_multi_destroy(vgx_reg_multi multi);
VGX_API int32_t vgx_reg_multi_num_shards(vgx_reg_multi multi);
/* How the contexts' results meet on context 0.  Default VGX_REDUCE_PEER_SUM (the name is round 2's: since
 * round 4 nothing is summed): context 0 GATHERS every constraint's [45] block from the context that computed
 * it, through xGMI peer mappings, and assembles the fused buffer once, in list order.
 * VGX_REDUCE_RCCL: ONE ncclAllReduce(sum) per solver evaluation over xGMI (BASELINE north_star) of the
 * [n][45] array of blocks (words summed as int64), every context contributing its own rows and zero bits
 * elsewhere -- the contributing context's bit pattern in any order
 * -- then the same assembly (librccl.so is opened at run time, one communicator per context from
 * ncclCommInitAll, so every context needs its own device; VGX_ERR_UNSUPPORTED if RCCL cannot be opened or two
 * contexts share a device).  Either way the buffer is the one a single vgx_reg_batch over the whole list
 * assembles, BIT FOR BIT, whatever the number of contexts and the placement. */
#define VGX_REDUCE_PEER_SUM 0
#define VGX_REDUCE_RCCL 1
VGX_API int vgx_reg_multi_set_reduction(vgx_reg_multi multi, int32_t reduction);
VGX_API int vgx_reg_multi_shard_of(vgx_reg_multi multi, int32_t* shard_of /* [n] */);
/* One solver evaluation: every context runs vgx_reg_batch_evaluate_normal on its share concurrently (own
 * thread, own stream); the per-constraint blocks meet on context 0 (see vgx_reg_multi_set_reduction), which
 * assembles the fused buffer of vgx_reg_batch_assemble's layout (vgx_reg_fused_size(n_nodes, n) doubles) in
 * list order and returns it to the host.  Bitwise reproducible and independent of the sharding.
 * status: [n], nullable.  A context whose evaluation fails fails the call with that context's message. */
VGX_API int vgx_reg_multi_evaluate_fused(vgx_reg_multi multi, const double* poses, int32_t n_nodes,
                                         double* fused_host, int32_t* status);
/* The same pass for solvers that want residual blocks (Ceres through vgx_reg_compress_normal): the
 * [n][45] normal blocks in the caller's constraint order; needs no reduction at all. */
VGX_API int vgx_reg_multi_evaluate_normal(vgx_reg_multi multi, const double* poses, int32_t n_nodes,
                                          double* normal_host /* [n][45] */, int32_t* status);
/* ... and its cost-only form (vgx_reg_batch_evaluate_cost on every context's share): cost_host[c] = element [0] of the
 * block above, bit for bit, in the caller's constraint order. */
VGX_API int vgx_reg_multi_evaluate_cost(vgx_reg_multi multi, const double* poses, int32_t n_nodes,
                                        double* cost_host /* [n] */, int32_t* status);

/* ---- overlap detection (callers' side of REG) -------------------------- */
/* VoxgraphSubmap::getSubmapFrameSurfaceObb (voxgraph_submap.cpp:280-321): box around the
 * kVoxels registration voxels (centres -+ half a voxel), submap frame.  Needs the
 * VGX_POINTS_VOXELS set.  Returns VGX_ERR_INVALID when the set is empty. */
VGX_API int vgx_submap_surface_obb(vgx_submap submap, float min_xyz[3], float max_xyz[3]);
/* VoxgraphSubmap::getMissionFrameSurfaceAabb = BoundingBox::getAabbFromObbAndPose
 * (bounding_box.cpp:28-42) for a 4-DoF pose {x,y,z,yaw}. */
VGX_API int vgx_submap_mission_surface_aabb(vgx_submap submap, const double pose[4],
                                            float min_xyz[3], float max_xyz[3]);
/* PoseGraphInterface::updateOverlappingSubmapList (pose_graph_interface.cpp:109-147) over
 * VoxgraphSubmap::overlapsWith (voxgraph_submap.cpp:245-278): all pairs i < j whose
 * mission-frame surface AABBs intersect and for which at least one isosurface block
 * centre of submap i, carried into submap j's frame, falls in an allocated block of j.
 * The AABB stage runs on the host, the block stage is one launch over the surviving pairs.
 * Needs both point sets on every submap.  pairs: [max_pairs][2] indices into `submaps`,
 * in the reference's loop order. */
VGX_API int vgx_find_overlapping_pairs(vgx_ctx ctx, int32_t n, const vgx_submap* submaps,
                                       const double* poses /* [n][4] */, int32_t* pairs,
                                       int32_t max_pairs, int32_t* n_pairs);

/* ---- TSDF: voxblox::FastTsdfIntegrator ---------------------------------- */
/* Replaces the integrator voxgraph constructs and drives at
 * voxgraph/src/frontend/measurement_processors/pointcloud_integrator.cpp:66-83
 * (`new voxblox::FastTsdfIntegrator(config, layer)`, `setLayer`,
 * `integratePointCloud(T_submap_sensor, pointcloud, colors)`).  The arithmetic is
 * voxblox's (not vendored in the reference; restated in oracle/tsdf_oracle.c). */
typedef struct vgx_tsdf_layer_s* vgx_tsdf_layer;           /* voxblox::Layer<TsdfVoxel> */
typedef struct vgx_tsdf_integrator_s* vgx_tsdf_integrator; /* voxblox::FastTsdfIntegrator */

/* voxblox::TsdfIntegratorBase::Config (voxblox defaults; voxgraph_mapper.yaml:21-28
 * overrides truncation 0.60, max ray 16 m, const weight, drop-off, sparsity
 * compensation 20).  integrator_threads / max_integration_time_s have no meaning on the GPU: every ray is
 * its own thread; integration_order_mode (voxgraph_mapper.yaml:29) is `integration_order` below. */
#define VGX_TSDF_ORDER_MIXED 0  /* integration_order_mode "mixed" (voxblox's and voxgraph's default) */
#define VGX_TSDF_ORDER_SORTED 1 /* "sorted": points visited by ascending squared norm of point_C    */
/* ABI note: the struct grew at its END in rounds 3 (deterministic) and 4 (integration_order), and every field is
 * validated (an integration_order that is neither value is refused with VGX_ERR_INVALID).  Fill it with
 * vgx_tsdf_config_default() -- or zero it -- before setting fields; a caller compiled against an older header must be
 * rebuilt (the library reads sizeof(vgx_tsdf_config) bytes). */
typedef struct vgx_tsdf_config {
  float default_truncation_distance;    /* 0.1   */
  float max_weight;                     /* 10000 */
  int32_t voxel_carving_enabled;        /* 1     */
  float min_ray_length_m;               /* 0.1   */
  float max_ray_length_m;               /* 5.0   */
  int32_t use_const_weight;             /* 0     */
  int32_t allow_clear;                  /* 1     */
  int32_t use_weight_dropoff;           /* 1     */
  int32_t use_sparsity_compensation_factor; /* 0 */
  float sparsity_compensation_factor;   /* 1.0   */
  float start_voxel_subsampling_factor; /* 2.0   */
  int32_t max_consecutive_ray_collisions; /* 2   */
  int32_t clear_checks_every_n_frames;  /* 1     */
  int32_t enable_anti_grazing;          /* 0     (merged integrator only) */
  /* 0: every ray is its own thread and rays race on the approximate sets and the voxels exactly as
   * voxblox's worker threads do (a legal order, different from run to run on dense scans).
   * 1: REPRODUCIBLE mode -- the scan is integrated as voxblox does with integrator_threads = 1 and
   * integration_order_mode "mixed": the same rays are cast, stop at the same voxel and update
   * every voxel in the same order, so the same scans give the same layer bit for bit, run after
   * run (and the layer oracle/tsdf_oracle.c computes).  Slower (several sorts and a fixed-point
   * iteration per scan instead of one kernel); meant for regression tests and reproducible maps. */
  int32_t deterministic;                /* 0     */
  /* voxblox's integration_order_mode: VGX_TSDF_ORDER_MIXED (1024-point groups visited round-robin) or
   * VGX_TSDF_ORDER_SORTED (ascending f32 squaredNorm() of the sensor-frame point; voxblox sorts with the
   * unstable std::sort, so the order of points at EQUAL range is unspecified there: here, and in the
   * oracle, equal ranges are visited by ascending point index).  The visiting order is what the
   * reproducible mode reproduces and what the merged integrator merges a group's points in; the racing
   * fast integrator (deterministic = 0) has no visiting order and ignores it. */
  int32_t integration_order;            /* 0     */
} vgx_tsdf_config;
VGX_API void vgx_tsdf_config_default(vgx_tsdf_config* cfg);

/* An active (unfinished) submap's TSDF layer, resident on the GPU between scans
 * (SURVEY.md 3.1).  Unbounded, like voxblox::Layer<TsdfVoxel>: blocks (12 B per voxel) are allocated
 * on demand wherever rays go.  lut_min / lut_dim (block coordinates; both may be NULL) and max_blocks
 * (<= 0: a default) are only an initial reservation: before each scan the integrator enlarges the
 * block table and the block pool, on the stream, to hold everything that scan can reach
 * (origin +- max_ray_length + truncation), so no update is ever dropped for lack of room.  If the
 * GPU itself runs out of memory the integrate call fails with VGX_ERR_NOMEM. */
VGX_API int vgx_tsdf_layer_create(vgx_ctx ctx, float voxel_size, int32_t voxels_per_side,
                                  const int32_t lut_min[3], const int32_t lut_dim[3],
                                  int32_t max_blocks, vgx_tsdf_layer* out);
VGX_API int vgx_tsdf_layer_destroy(vgx_tsdf_layer layer);
/* allocated blocks; *dropped_updates = voxel updates that found no block (always 0 unless an
 * allocation failed, in which case the next integrate call reports VGX_ERR_NOMEM).  Waits for the
 * scans in flight. */
VGX_API int vgx_tsdf_layer_stats(vgx_tsdf_layer layer, int32_t* n_blocks,
                                 int64_t* dropped_updates);
/* Optional: make room NOW for scans taken from around `origin` (layer frame) that reach up to
 * reach_m metres (max_ray_length + truncation), so that the first scans there do not pay for the
 * enlargement.  Scans reserve for themselves anyway. */
VGX_API int vgx_tsdf_layer_reserve(vgx_tsdf_layer layer, const float origin[3], float reach_m);
/* Acknowledges dropped updates (the GPU ran out of memory during an earlier scan: integrate calls keep
 * failing with VGX_ERR_NOMEM until then) and resets the counter, after the caller has made room or
 * decided to live with the hole.  Waits for the scans in flight. */
VGX_API int vgx_tsdf_layer_clear_dropped(vgx_tsdf_layer layer);
/* how often the layer has enlarged its block table or pool so far (diagnostics) */
VGX_API int64_t vgx_tsdf_layer_growths(vgx_tsdf_layer layer);
/* block_index[n][3], distance / weight [n][vps^3], rgba [n][vps^3][4]; any may be NULL */
VGX_API int vgx_tsdf_layer_download(vgx_tsdf_layer layer, int32_t* block_index,
                                    float* distance, float* weight, uint8_t* rgba);
/* Replaces the layer's contents with host blocks in the same layout (rgba may be NULL): hands a
 * voxblox::Layer<TsdfVoxel> that already holds data over to the GPU integrator. */
VGX_API int vgx_tsdf_layer_upload(vgx_tsdf_layer layer, int32_t n_blocks, const int32_t* block_index,
                                  const float* distance, const float* weight, const uint8_t* rgba);

VGX_API int vgx_tsdf_integrator_create(vgx_ctx ctx, const vgx_tsdf_config* cfg,
                                       vgx_tsdf_layer layer, vgx_tsdf_integrator* out);
VGX_API int vgx_tsdf_integrator_destroy(vgx_tsdf_integrator integrator);
/* FastTsdfIntegrator::setLayer (pointcloud_integrator.cpp:77) */
VGX_API int vgx_tsdf_integrator_set_layer(vgx_tsdf_integrator integrator, vgx_tsdf_layer layer);
/* Optional hint: the scans to come are ORGANISED clouds of `width` points per row (sensor_msgs/PointCloud2.width, which
 * voxgraph's callback receives -- pointcloud_integrator.cpp:23 -- and voxblox's flat Pointcloud drops; 0 = unorganised, the
 * default).  The racing integrator then gives a workgroup a 16 x 16 tile of beams instead of 256 consecutive ones: the
 * beams that end in one voxel are neighbours in both directions, so most of a voxel's updates meet inside one workgroup.
 * Only the assignment of points to workgroups depends on it -- which rays are cast and what they write is one of voxblox's
 * legal orders either way; a scan whose length is not a multiple of `width` is treated as unorganised. */
VGX_API int vgx_tsdf_integrator_set_cloud_width(vgx_tsdf_integrator integrator, int32_t width);
/* integratePointCloud(T_G_C, points_C, colors, freespace_points)
 * (pointcloud_integrator.cpp:83).  T_G_C = {qw,qx,qy,qz, tx,ty,tz} f32
 * (voxblox::Transformation); points_C [n][3] sensor frame; rgba [n][4] or NULL.
 * Host pointers (pageable is fine: the arrays are read before the call returns, through pinned staging buffers of the
 * integrator's own, and are the caller's again afterwards).  n_updates == NULL -- what voxblox's void call corresponds to:
 * the call returns with the scan QUEUED on the context's TSDF stream; the layer is the device's, and every reader of it
 * (vgx_tsdf_layer_download / _stats, vgx_submap_from_tsdf_layer, the next scan) is ordered behind the scan on that stream;
 * vgx_ctx_synchronize_tsdf waits for it explicitly.  n_updates != NULL: a COUNTED scan -- the call waits for it and
 * returns the number of voxel updates performed (a slower kernel instantiation: diagnostics, tests). */
VGX_API int vgx_tsdf_integrate(vgx_tsdf_integrator integrator, const float T_G_C[7],
                               const float* points_C, const uint8_t* rgba, int64_t n,
                               int32_t freespace_points, int64_t* n_updates);
/* Same with DEVICE pointers (scan already resident in HBM); asynchronous unless
 * n_updates != NULL. */
VGX_API int vgx_tsdf_integrate_device(vgx_tsdf_integrator integrator, const float T_G_C[7],
                                      const void* d_points_C, const void* d_rgba, int64_t n,
                                      int32_t freespace_points, int64_t* n_updates);

/* voxblox::MergedTsdfIntegrator::integratePointCloud (north_star names it; voxgraph itself
 * constructs the Fast integrator, pointcloud_integrator.h:30) on the same integrator object -- config
 * and layer; the approximate sets of the fast integrator are not involved: the valid points are
 * grouped by the voxel their end point falls in (clearing rays separately), every group is merged
 * into one weighted-mean point in the reference's visiting order and ONE ray is cast for it through
 * all its voxels with the summed weight; with enable_anti_grazing a ray skips voxels that are the end
 * voxel of another group.  Same argument conventions as vgx_tsdf_integrate[_device].
 * Inputs the reference leaves undefined (all integrators): a coordinate that is NaN indexes voxel 0 on its axis,
 * one beyond +-2^31 voxels saturates (getGridIndexFromPoint's cast, defined the same way in oracle/tsdf_oracle.c);
 * such points pass isPointValid as in the reference and, where they are clearing rays (allow_clear / freespace
 * scans), carve along their direction up to max_ray_length_m like any other return beyond the range.
 * VGX_ERR_UNSUPPORTED: a ray of more than 2^24 voxel steps; a voxel beyond +-2^20 voxels of the layer origin on a
 * ray's walk (reproducible mode and merged integrator). */
VGX_API int vgx_tsdf_integrate_merged(vgx_tsdf_integrator integrator, const float T_G_C[7],
                                      const float* points_C, const uint8_t* rgba, int64_t n,
                                      int32_t freespace_points, int64_t* n_updates);
VGX_API int vgx_tsdf_integrate_merged_device(vgx_tsdf_integrator integrator, const float T_G_C[7],
                                             const void* d_points_C, const void* d_rgba, int64_t n,
                                             int32_t freespace_points, int64_t* n_updates);

/* ---- Scans: a raw sensor_msgs/PointCloud2 decoded on the device ------------------ */
/* What PointcloudIntegrator::integratePointcloud does on the host before it reaches the integrator
 * (pointcloud_integrator.cpp:29-63): pcl::fromROSMsg into a PointXYZ / PointXYZI / PointXYZRGB cloud and
 * voxblox::convertPointcloud, which drops the points that are not finite and makes one colour per kept point.  A vgx_scan
 * holds the result on the device -- the kept points [n][3] f32 and their colours [n][4] u8, in message order -- and the
 * integrators take it as it is.  The caller resolves the message's field names to byte offsets (vgx_scan_layout; the C++
 * mirror gpu_pointcloud_integrator.h does it from a message).  PCL and voxblox_ros are not vendored: every colour rule
 * and the filter are [recalled] from voxblox_ros/conversions.h, voxblox/utils/color_maps.h and PCL's point layouts.
 * Rules (what the kernel, vgx_scan.hip, and tests/scan_msg_ref.py both follow; f32, no contraction):
 *   addressing  point i = r * width + c lies at data + r * row_step + c * point_step; fields are little-endian.  Any
 *               point_step >= 1 and any offsets whose 4 bytes fit in point_step are legal: unaligned fields, overlapping
 *               fields and padded rows included.  When data, point_step, row_step and the offsets are all multiples of
 *               4 the kernel loads dwords, else it assembles every field from byte loads; the result is the same.
 *   filter      kept iff isfinite(x) && isfinite(y) && isfinite(z) (convertPointcloud's isPointFinite [recalled]); the
 *               three floats are copied bit for bit (-0.0 stays -0.0).  Kept points stay in ascending i: the order the
 *               reproducible mode visits them in and the one that decides which point takes a start voxel.
 *               n_dropped = width * height - n_points.
 *   colour      VGX_SCAN_COLOR_RGB: bytes b0 b1 b2 b3 at color_offset give rgba = (b2, b1, b0, b3) -- PCL's packed
 *               0xAARRGGBB and Color(p.r, p.g, p.b, p.a).  VGX_SCAN_COLOR_INTENSITY: v the f32 at color_offset;
 *               v = (min < v) ? v : min; v = (v < max) ? v : max (std::max(min, v), std::min(max, .) with their argument
 *               order: NaN becomes min); h = (v - min) / (max - min) in f32; g = (uint8) std::round((double)h * 255.0)
 *               (grayColorMap); rgba = (g, g, g, 255).  VGX_SCAN_COLOR_NONE: every kept point gets constant_rgba.
 * Refused with VGX_ERR_INVALID before anything is uploaded or launched, the scan keeping what it held (vgx_last_error
 * says which): NULL arguments, a scan of another context, point_step == 0, a field whose 4 bytes do not fit in
 * point_step, row_step < width * point_step, an unknown color_kind, n_bytes < (height - 1) * row_step + width *
 * point_step when width * height > 0, an intensity range that is not finite or not max > min (the decode
 * calls check it, whatever the color_kind).  VGX_ERR_UNSUPPORTED: is_bigendian != 0; width * height >= 2^31.  Coordinates that are not FLOAT32 cannot be
 * expressed in the layout.  width * height == 0, or a cloud whose every point is dropped: VGX_OK and 0 points;
 * integrating such a scan is the empty scan of vgx_tsdf_integrate.  Out of device memory: VGX_ERR_NOMEM, and the handle
 * then holds no scan (stats report 0).
 * Streams: decoding runs on the context's TSDF stream under the TSDF lock: the upload (host variant: through two pinned
 * staging buffers filled in turn, so that the host copy of one piece overlaps the upload of the piece before; pageable
 * memory where no pinned memory is to be had), ONE kernel whatever the size -- the compaction's prefix sum is taken inside
 * the launch -- and a 16-byte read-back of the kept-point count, which is the call's one host synchronisation.
 * vgx_scan_stats costs nothing afterwards.  The arrays hold width * height points' room and grow on demand behind a
 * stream synchronisation.  vgx_tsdf_integrate[_merged]_scan is vgx_tsdf_integrate[_merged]_device on the scan's arrays
 * and count: n_updates == NULL returns with the scan queued, and because decode and integration share a stream the handle
 * may be decoded into again as soon as the integrate call has returned.  One call at a time per handle. */
#define VGX_SCAN_COLOR_NONE 0      /* pcl::PointXYZ */
#define VGX_SCAN_COLOR_RGB 1       /* pcl::PointXYZRGB: 4 bytes at color_offset */
#define VGX_SCAN_COLOR_INTENSITY 2 /* pcl::PointXYZI: FLOAT32 at color_offset */
/* the sensor_msgs/PointCloud2 header with the field names resolved to byte offsets inside a point */
typedef struct vgx_scan_layout {
  uint32_t width, height, point_step, row_step;
  uint32_t offset_x, offset_y, offset_z; /* FLOAT32 each */
  int32_t color_kind;                    /* VGX_SCAN_COLOR_* */
  uint32_t color_offset;                 /* not read for VGX_SCAN_COLOR_NONE */
  int32_t is_bigendian;
} vgx_scan_layout;
/* Fill it with vgx_scan_config_default() before setting fields; every field is validated. */
typedef struct vgx_scan_config {
  float intensity_min, intensity_max; /* 0, 10000: GrayscaleColorMap with setMaxValue(10000.0) (pointcloud_integrator.cpp:12-14) */
  uint8_t constant_rgba[4];           /* 0, 0, 0, 0: the colour of a cloud without colours, a default voxblox::Color [recalled] */
} vgx_scan_config;
typedef struct vgx_scan_s* vgx_scan;
VGX_API void vgx_scan_config_default(vgx_scan_config* cfg);
/* HOST ONLY (no device, no context): VGX_OK, or the code a decode of n_bytes bytes in this layout is refused with.  It
 * takes no config: the intensity range is checked by the decode calls alone. */
VGX_API int vgx_scan_layout_check(const vgx_scan_layout* layout, int64_t n_bytes);
VGX_API int vgx_scan_create(vgx_ctx ctx, vgx_scan* out);
VGX_API int vgx_scan_destroy(vgx_scan scan);
/* data: the message's bytes in host memory (pageable is fine: they are read before the call returns); cfg == NULL: the
 * defaults.  Returns with the scan decoded and counted. */
VGX_API int vgx_scan_decode_msg(vgx_scan scan, const vgx_scan_layout* layout, const vgx_scan_config* cfg, const void* data,
                                int64_t n_bytes);
/* the same with the message already in DEVICE memory, ready with respect to the TSDF stream (vgx_ctx_tsdf_wait_for_stream) */
VGX_API int vgx_scan_decode_msg_device(vgx_scan scan, const vgx_scan_layout* layout, const vgx_scan_config* cfg,
                                       const void* d_data, int64_t n_bytes);
/* either may be NULL; no device work */
VGX_API int vgx_scan_stats(vgx_scan scan, int64_t* n_points, int64_t* n_dropped);
/* points [n][3] f32, rgba [n][4] u8; either may be NULL.  Waits for the TSDF stream. */
VGX_API int vgx_scan_download(vgx_scan scan, float* points, uint8_t* rgba);
/* DEVICE pointers to the same arrays (NULL for a scan of 0 points); valid until the next decode into the handle or its
 * destruction.  Either may be NULL. */
VGX_API int vgx_scan_device_pointers(vgx_scan scan, const void** d_points, const void** d_rgba);
/* vgx_tsdf_integrate_device / vgx_tsdf_integrate_merged_device on the scan's points, colours and count */
VGX_API int vgx_tsdf_integrate_scan(vgx_tsdf_integrator integrator, const float T_G_C[7], vgx_scan scan,
                                    int32_t freespace_points, int64_t* n_updates);
VGX_API int vgx_tsdf_integrate_merged_scan(vgx_tsdf_integrator integrator, const float T_G_C[7], vgx_scan scan,
                                           int32_t freespace_points, int64_t* n_updates);

/* ---- Scan undistortion: a sweep moved into one frame by a pose track, inside the decode ---- */
/* The reference's demo feeds voxgraph a cloud that lidar_undistortion has corrected (arche_demo.launch:6,12).  That
 * package is not vendored: the rules below are DEFINED here, chosen so that a caller who makes every distinct stamp a
 * knot gets one rigid transform per stamp.  vgx_scan_decode_msg_undistorted is vgx_scan_decode_msg with one more step
 * per point: its time field picks a segment of the track and the point is moved from the sensor frame at its own time
 * into the sensor frame at the scan's reference time.  Rules (what the kernel, vgx_scan.hip, and
 * tests/scan_undistort_ref.py both follow; f32 unless it says f64, no contraction):
 *   time field  kind UINT32 / FLOAT32 / FLOAT64: 4 / 4 / 8 little-endian bytes at `offset`, which must fit in point_step
 *               and may be unaligned (under the dword path an 8-byte field is read as two words).
 *               t = offset_s + (double)raw * scale: one rounded f64 multiply, then one rounded f64 add.
 *   track       knot_T [n_knots][7] qw,qx,qy,qz, tx,ty,tz holds T_ref_sensor(knot_time[k]): the sensor at knot time k
 *               expressed in the sensor frame at the scan's reference time.  Both arrays are HOST arrays and have been
 *               read when the call returns.  1 <= n_knots <= 65536, the times finite and strictly ascending, every
 *               knot_T entry finite.  Quaternions are not normalised by the library.
 *   segment     k = (number of knots with knot_time <= t) - 1.  t < knot_time[0]: k = 0, a = 0, the point counts as
 *               clamped.  t > knot_time[K-1]: k = K-1, a = 0, clamped.  t == knot_time[K-1]: k = K-1, a = 0, not clamped.
 *               Otherwise a = (float)((t - t_k) / (t_{k+1} - t_k)), the subtractions and the division in f64.
 *   point       g0 = knot k applied to p as the integrators apply T_G_C (Eigen's quaternion-vector product plus the
 *               translation: uv = 2 (q x p), g = (p + qw uv + q x uv) + t, in that association).  a == 0.0f: the output is
 *               g0 and knot k+1 is not evaluated.  Otherwise g1 = knot k+1 applied to p and out = g0 + a * (g1 - g0) per
 *               component: exact in translation, chordal in rotation, no slerp and no transcendental.
 *   filter      in this order: x, y, z finite as the plain decode tests them, else dropped (not finite); t finite, else
 *               dropped (bad time); all three outputs finite, else dropped (overflowed).  Kept points stay in message
 *               order, a vgx_scan still never holds a non-finite point, colours follow the plain decode unchanged.
 *               (With an identity knot a kept -0.0 coordinate comes back as +0.0: it went through the arithmetic.)
 * Refused with VGX_ERR_INVALID, the scan keeping what it held (vgx_last_error says which): NULL arguments, an unknown time
 * kind, a time field that does not fit in point_step, scale or offset_s not finite, n_knots out of range, knot times not
 * finite or not strictly ascending, a knot_T entry that is not finite, and everything the plain decode refuses.
 * Streams: as the plain decode -- ONE kernel and ONE host synchronisation.  The knots go up as asynchronous copies on the
 * TSDF stream ahead of the launch into a buffer the handle owns (it grows on demand behind a stream synchronisation); the
 * three counters come back in the decode's one read-back, 40 bytes instead of 16. */
#define VGX_SCAN_TIME_UINT32 0  /* e.g. Ouster's "t": nanoseconds since the sweep's start */
#define VGX_SCAN_TIME_FLOAT32 1 /* e.g. Velodyne's "time": seconds */
#define VGX_SCAN_TIME_FLOAT64 2 /* e.g. an absolute "timestamp" in seconds */
#define VGX_SCAN_TRACK_MAX_KNOTS 65536
typedef struct vgx_scan_time_field {
  int32_t kind;    /* VGX_SCAN_TIME_* */
  uint32_t offset; /* byte offset inside a point */
  double scale;    /* seconds per unit of the raw value */
  double offset_s; /* added after scaling */
} vgx_scan_time_field;
typedef struct vgx_scan_track {
  int32_t n_knots;
  const double* knot_time; /* HOST [n_knots] */
  const float* knot_T;     /* HOST [n_knots][7] */
} vgx_scan_track;
/* HOST ONLY (no device, no context): VGX_OK, or the code an undistorting decode of n_bytes bytes is refused with */
VGX_API int vgx_scan_undistort_check(const vgx_scan_layout* layout, const vgx_scan_time_field* time_field,
                                     const vgx_scan_track* track, int64_t n_bytes);
VGX_API int vgx_scan_decode_msg_undistorted(vgx_scan scan, const vgx_scan_layout* layout, const vgx_scan_config* cfg,
                                            const vgx_scan_time_field* time_field, const vgx_scan_track* track,
                                            const void* data, int64_t n_bytes);
/* the same with the message already in DEVICE memory (the track's arrays stay host arrays) */
VGX_API int vgx_scan_decode_msg_undistorted_device(vgx_scan scan, const vgx_scan_layout* layout, const vgx_scan_config* cfg,
                                                   const vgx_scan_time_field* time_field, const vgx_scan_track* track,
                                                   const void* d_data, int64_t n_bytes);
/* Of the last decode: points dropped for a time that is not finite, points dropped because an output was not finite, kept
 * points whose time lay outside the track.  Zeros after a plain decode.  vgx_scan_stats' n_dropped is the sum of all
 * three drop reasons (not finite + bad time + overflowed).  Any may be NULL; no device work. */
VGX_API int vgx_scan_undistort_stats(vgx_scan scan, int64_t* n_bad_time, int64_t* n_overflowed, int64_t* n_clamped);

/* ---- Depth-image scans: a sensor_msgs/Image depth frame unprojected, coloured and filtered inside the decode ---- */
/* An RGB-D driver publishes a depth image (16UC1 counts or 32FC1 metres) with a CameraInfo and usually a registered colour
 * image, not a cloud.  vgx_scan_decode_depth_image fills a vgx_scan from those: what depth_image_proc's point_cloud_xyz[rgb]
 * nodelet followed by the PointCloud2 decode would leave, without the cloud ever existing.  Afterwards the handle is
 * what it is after vgx_scan_decode_msg -- vgx_scan_stats / _download / _device_pointers, vgx_tsdf_integrate[_merged]_scan
 * and vgx_scan_registration_set_scan behave alike -- and a handle may be decoded into by any decode kind in turn.
 * depth_image_proc is not vendored: the rules are DEFINED here, and where one is modelled on it, it says [recalled].
 * Rules (what the kernel, vgx_scan.hip, and tests/depth_image_ref.py both follow; f32 with one rounding per operation,
 * no contraction, unless it says f64):
 *   candidates  pixel (u, v) is a candidate iff u % stride_u == 0 && v % stride_v == 0.  wc = ceil(width / stride_u),
 *               hc = ceil(height / stride_v), candidate i = (v / stride_v) * wc + (u / stride_u), n_candidates = wc * hc.
 *               Kept points stay in ascending i: image row-major order, the order the reproducible integrator visits them in.
 *   depth       16UC1: raw = the two little-endian bytes at depth + v * row_step + 2 u, z = (float)raw * depth_unit_m.
 *               32FC1: z = the float whose four little-endian bytes lie at depth + v * row_step + 4 u.  Any row_step >=
 *               width * bytes per pixel and any base address are legal; when the base and row_step are multiples of the
 *               element size the kernel loads elements, else it assembles them from bytes; the result is the same.
 *   filter      in this order, one counter each (vgx_scan_depth_stats):
 *               1. invalid unless 0 < z && z < +inf.  For 16UC1 that is raw != 0, depth_image_proc's rule [recalled]; for
 *                  32FC1 it also drops 0, -0 and negatives, which depth_image_proc keeps: a stated deviation (a point at
 *                  or behind the optical centre is no measurement).
 *               2. out of range unless min_depth_m <= z && z <= max_depth_m.
 *               3. x = (((float)u - cxf) * z) * kx, y = (((float)v - cyf) * z) * ky with cxf = (float)cx, cyf = (float)cy,
 *                  kx = (float)(1.0 / fx), ky = (float)(1.0 / fy): each formed on the host in f64 and rounded once.  The
 *                  point is (x, y, z) in the optical frame (z forward, x right, y down).
 *               4. overflowed unless x and y are finite.
 *   track step  (the undistorting forms) for a point that survived: t = offset_s + (double)v * scale with v the row in the
 *               full image, one rounded f64 multiply then one rounded f64 add; the segment, point and remaining filter
 *               rules of "Scan undistortion" apply word for word (bad time, then overflowed after the track), counted by
 *               vgx_scan_undistort_stats as they are there.  vgx_scan_depth_stats' n_overflowed counts step 4 only.
 *   counters    vgx_scan_stats' n_dropped = n_candidates - n_points, the sum of all drop reasons (pixels the strides skip
 *               are not drops).  vgx_scan_undistort_stats reports zeros after a depth decode without a track,
 *               vgx_scan_depth_stats reports zeros after a PointCloud2 decode.
 *   colour      of a kept point, from the bytes b0.. of the pixel at color + v * color_row_step + u * bytes per pixel:
 *               RGB8 (b0, b1, b2, 255), BGR8 (b2, b1, b0, 255), RGBA8 (b0, b1, b2, b3), BGRA8 (b2, b1, b0, b3), MONO8
 *               (b0, b0, b0, 255); NONE: vgx_scan_config.constant_rgba.  The config's intensity range is validated as the
 *               other decodes validate it and is otherwise unused.
 * Refused with VGX_ERR_INVALID before anything is uploaded or launched, the scan keeping what it held (vgx_last_error
 * says which): NULL arguments (cfg may be NULL: the defaults), a colour image that is NULL while color_kind is not NONE,
 * an unknown encoding or colour kind, row_step < width * bytes per pixel and the same for the colour image, n_bytes <
 * (height - 1) * row_step + width * bytes per pixel when width * height > 0 for either image, fx or fy zero or not finite,
 * cx or cy not finite, depth_unit_m not finite or <= 0 (16UC1), a NaN depth bound, min_depth_m < 0, min_depth_m >
 * max_depth_m, a stride < 1, an intensity range the other decodes refuse, a row time whose scale or offset_s is not
 * finite, and everything vgx_scan_undistort_check refuses in a track.  VGX_ERR_UNSUPPORTED: is_bigendian != 0; width *
 * height >= 2^31.  width * height == 0, or every candidate dropped: VGX_OK and 0 points.  Out of device memory:
 * VGX_ERR_NOMEM, and the handle then holds no scan.
 * Streams and cost are the PointCloud2 decode's: the TSDF stream under the TSDF lock; the host forms upload the depth
 * image and then the colour image through the handle's two pinned staging buffers filled in turn; ONE kernel whatever the
 * size (tiles of 1024 consecutive candidates, four per thread, ranked inside the workgroup and along the tile chain: no
 * atomic decides a position); ONE read-back of the counters (64 bytes), the call's one host synchronisation.  One call at
 * a time per handle. */
#define VGX_DEPTH_16UC1 0 /* uint16 counts, also "mono16" */
#define VGX_DEPTH_32FC1 1 /* float32 metres */
#define VGX_IMAGE_COLOR_NONE 0
#define VGX_IMAGE_COLOR_RGB8 1
#define VGX_IMAGE_COLOR_BGR8 2
#define VGX_IMAGE_COLOR_RGBA8 3
#define VGX_IMAGE_COLOR_BGRA8 4
#define VGX_IMAGE_COLOR_MONO8 5
typedef struct vgx_depth_image_layout {
  uint32_t width, height, row_step; /* the depth image; row_step in bytes */
  int32_t encoding;                 /* VGX_DEPTH_* */
  int32_t is_bigendian;
  int32_t color_kind;               /* VGX_IMAGE_COLOR_*; the colour image has the depth image's width and height */
  uint32_t color_row_step;          /* not read for VGX_IMAGE_COLOR_NONE */
} vgx_depth_image_layout;
/* Fill it with vgx_depth_camera_default() before setting fields (fx, fy have no default); every field is validated. */
typedef struct vgx_depth_camera {
  double fx, fy, cx, cy;          /* CameraInfo K[0], K[4], K[2], K[5] of the RECTIFIED depth image */
  float depth_unit_m;             /* 0.001: metres per count of a 16UC1 image; not read for 32FC1 */
  float min_depth_m, max_depth_m; /* 0, +inf: the z-depth gate, both ends included */
  int32_t stride_u, stride_v;     /* 1, 1: every stride-th column / row */
} vgx_depth_camera;
/* a rolling shutter's time of image row v: t = offset_s + (double)v * scale, in the track's time */
typedef struct vgx_depth_row_time {
  double scale, offset_s;
} vgx_depth_row_time;
VGX_API void vgx_depth_camera_default(vgx_depth_camera* camera);
/* HOST ONLY (no device, no context): VGX_OK, or the code a decode of these byte counts is refused with.  It takes no
 * config: the intensity range is checked by the decode calls alone.  color_n_bytes is not read for VGX_IMAGE_COLOR_NONE. */
VGX_API int vgx_depth_image_check(const vgx_depth_image_layout* layout, const vgx_depth_camera* camera, int64_t depth_n_bytes,
                                  int64_t color_n_bytes);
/* ... and the code an undistorting decode is refused with */
VGX_API int vgx_depth_image_undistort_check(const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                            const vgx_depth_row_time* row_time, const vgx_scan_track* track,
                                            int64_t depth_n_bytes, int64_t color_n_bytes);
/* depth, color: the images' bytes in host memory (pageable is fine: they are read before the call returns); color is not
 * read for VGX_IMAGE_COLOR_NONE; cfg == NULL: the defaults.  Returns with the scan decoded and counted. */
VGX_API int vgx_scan_decode_depth_image(vgx_scan scan, const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                        const vgx_scan_config* cfg, const void* depth, int64_t depth_n_bytes,
                                        const void* color, int64_t color_n_bytes);
/* the same with both images already in DEVICE memory, ready with respect to the TSDF stream (vgx_ctx_tsdf_wait_for_stream) */
VGX_API int vgx_scan_decode_depth_image_device(vgx_scan scan, const vgx_depth_image_layout* layout,
                                               const vgx_depth_camera* camera, const vgx_scan_config* cfg, const void* d_depth,
                                               int64_t depth_n_bytes, const void* d_color, int64_t color_n_bytes);
/* the same with the track step: a rolling-shutter frame taken while the camera moved (the track's arrays are HOST arrays) */
VGX_API int vgx_scan_decode_depth_image_undistorted(vgx_scan scan, const vgx_depth_image_layout* layout,
                                                    const vgx_depth_camera* camera, const vgx_scan_config* cfg,
                                                    const vgx_depth_row_time* row_time, const vgx_scan_track* track,
                                                    const void* depth, int64_t depth_n_bytes, const void* color,
                                                    int64_t color_n_bytes);
VGX_API int vgx_scan_decode_depth_image_undistorted_device(vgx_scan scan, const vgx_depth_image_layout* layout,
                                                           const vgx_depth_camera* camera, const vgx_scan_config* cfg,
                                                           const vgx_depth_row_time* row_time, const vgx_scan_track* track,
                                                           const void* d_depth, int64_t depth_n_bytes, const void* d_color,
                                                           int64_t color_n_bytes);
/* Of the last decode: the pixels the strides kept, and of those the ones dropped as invalid, as out of range and because
 * x or y was not finite.  Zeros after a PointCloud2 decode.  Any may be NULL; no device work. */
VGX_API int vgx_scan_depth_stats(vgx_scan scan, int64_t* n_candidates, int64_t* n_invalid, int64_t* n_out_of_range,
                                 int64_t* n_overflowed);

/* ---- Projective depth-image integration: every voxel in view looks up ONE pixel and updates itself ---- */
/* The way dense RGB-D mappers integrate a frame (KinectFusion; voxblox's ProjectiveTsdfIntegrator [recalled]): no cloud, no
 * rays.  A gather -- one lane owns a voxel -- so nothing races, nothing is sorted and no approximate set is asked: the same
 * frames give the same layer, block order included, bit for bit on every run.  Neither project is vendored: the rules are
 * DEFINED here (what the kernel, vgx_projective.hip, and tests/projective_ref.py both follow; f32 with one rounding per
 * operation, no contraction, unless it says f64).  The integrator, its vgx_tsdf_config and its layer are the existing ones.
 * Config fields READ: default_truncation_distance (trunc), max_weight, voxel_carving_enabled, min_ray_length_m,
 * max_ray_length_m, use_const_weight, allow_clear, use_weight_dropoff.  NOT read: use_sparsity_compensation_factor,
 * sparsity_compensation_factor, start_voxel_subsampling_factor, max_consecutive_ray_collisions,
 * clear_checks_every_n_frames, enable_anti_grazing, deterministic, integration_order.  Of vgx_depth_camera the strides are
 * validated and otherwise not read: every pixel can be looked up.
 *   candidates  vgx_tsdf_projective_box, on the host in f64: reach = min(max_depth_m, max_ray_length_m) + trunc (an
 *               infinite max_depth_m is bounded by max_ray_length_m), taken as a Z-DEPTH.  The box is the axis-aligned box,
 *               in the layer frame, of the camera centre and of the four points P = ((u - cx) / fx * reach, (v - cy) / fy *
 *               reach, reach) for (u, v) in {-0.5, width - 0.5} x {-0.5, height - 0.5} (the corners of the area whose
 *               pixels can be looked up), each moved by T_G_C as below (uv = qv x P, uv += uv, cc = qv x uv, (P + qw uv +
 *               cc) + t).  Every voxel the rules can update has z <= reach (gates 3 and 4: z <= d + trunc and z <= r_v <= r_s + trunc;
 *               a clearing one: r_v <= max_ray_length_m - trunc < r_s, so z < d) and lies in that pyramid.  [A ray RANGE of `reach` along
 *               the corner rays would not contain them: the on-axis voxel at range reach lies beyond the corner points' plane.]
 *               lo = floor(min / bs) - 1, hi = floor(max / bs) + 1 per axis with bs = (double)voxel_size * voxels_per_side:
 *               the blocks that hold the extremes, widened by one block on every side.  Candidates are the blocks of
 *               [lo, hi] in ascending (z, y, x) order; n_candidate_blocks counts all of them (the kernel rejects whole
 *               blocks that provably find no pixel before it looks at their voxels; that changes no value and no count).
 *   voxel       global index (vx, vy, vz) = block * voxels_per_side + local; centre g = ((float)v + 0.5f) * voxel_size per axis.
 *   camera      p = g - t per axis, then rotated by the conjugate quaternion qv = (-qx, -qy, -qz), qw in the operation order
 *               of the library's transforms: uv = qv x p (each component a b - c d), uv += uv, cc = qv x uv, and
 *               (x, y, z) = (p + qw * uv) + cc.  The quaternion is used as given (not normalised).
 *   pixel       no update unless z > 0.  uf = (x / z) * (float)fx + (float)cx, vf = (y / z) * (float)fy + (float)cy;
 *               accepted iff 0 <= uf + 0.5f < (float)width and 0 <= vf + 0.5f < (float)height, tested in f32 before any
 *               cast; ui = floorf(uf + 0.5f), vi = floorf(vf + 0.5f).  Nearest pixel only.
 *   depth       d = the z of pixel (ui, vi) by the decode's depth rule; no update unless it passes the decode's filter
 *               rules 1 (0 < d < +inf) and 2 (min_depth_m <= d <= max_depth_m).
 *   ranges      r_v = sqrtf(x x + y y + z z) (summed left to right), s = r_v / z, r_s = d * s, sdf = (d - z) * s.
 *   gates       in this order: 1. r_s < min_ray_length_m: no update.  2. r_s > max_ray_length_m: a clearing pixel -- an
 *               update only if allow_clear && voxel_carving_enabled && r_v + trunc <= max_ray_length_m, with sdf =
 *               max_ray_length_m - r_v, counted in n_cleared; the gates below are not asked.  3. sdf < -trunc: no
 *               update.  4. sdf > trunc: an update only if voxel_carving_enabled, the sdf as it is, counted in n_carved.
 *   weight      w = use_const_weight ? 1 : 1.0f / (d * d); if use_weight_dropoff && sdf < -voxel_size:
 *               w = fmaxf((w * (trunc + sdf)) / (trunc - voxel_size), 0).  No sparsity factor.
 *   update      updateTsdfVoxel as every integrator here applies it: W = w_old + w; nothing changes if W < 1e-6f; else
 *               distance = clamp((sdf * w + d_old * w_old) / W, -trunc, trunc), the colour blended (Color::blendTwoColors
 *               with weights w_old, w) only where |sdf| < trunc, weight = fminf(max_weight, W).  A voxel of a block the layer
 *               does not hold is (0, 0, colour 0).  n_updates counts the voxels that changed (W >= 1e-6f); n_carved and
 *               n_cleared count those of them that came through gate 4 / gate 2.
 *   colour      of the incoming update: the registered colour image's pixel (ui, vi) by the decode's colour rule; with
 *               VGX_IMAGE_COLOR_NONE opaque white (255, 255, 255, 255).
 *   blocks      a block is allocated iff at least one of its voxels changed in this frame.  New blocks take pool slots in
 *               ascending candidate order behind the blocks the layer already held (n_new_blocks of them).
 * Validation is vgx_depth_image_check's, word for word, plus NULL handle / pose / image as the decode refuses them, before
 * anything is uploaded or launched; width * height == 0: VGX_OK, nothing done.  A pose that is not finite: VGX_ERR_INVALID;
 * width or height >= 2^24, both max_depth_m and max_ray_length_m unbounded, a box beyond +-2^30 blocks or of more than 2^24 blocks, or one the
 * layer's block table cannot hold (2^28 cells): VGX_ERR_UNSUPPORTED, as the other integrators refuse such a reach.
 * Streams and cost: the TSDF stream under the TSDF lock, one frame at a time per integrator; the host form uploads the
 * depth image and then the colour image through the integrator's two pinned staging buffers filled in turn.  Room for every
 * candidate block is reserved first: that reads the layer's exact block count behind everything queued -- the frame's ONE
 * host synchronisation, before the upload.  Then ONE kernel whatever the size.  counts == NULL: the call returns with the
 * frame QUEUED; with counts one read-back (56 bytes) more, and the call waits for the frame. */
typedef struct vgx_projective_counts { /* of the last frame */
  int64_t n_candidate_blocks, n_new_blocks, n_updates, n_carved, n_cleared;
} vgx_projective_counts;
/* depth, color: the images' bytes in host memory (read before the call returns); color is not read for VGX_IMAGE_COLOR_NONE */
VGX_API int vgx_tsdf_integrate_depth_image(vgx_tsdf_integrator integrator, const float T_G_C[7],
                                           const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                           const void* depth, int64_t depth_n_bytes, const void* color, int64_t color_n_bytes,
                                           vgx_projective_counts* counts /* NULL: queued, not waited for */);
/* the same with both images already in DEVICE memory, ready with respect to the TSDF stream; they are read until the frame
 * has run */
VGX_API int vgx_tsdf_integrate_depth_image_device(vgx_tsdf_integrator integrator, const float T_G_C[7],
                                                  const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                                  const void* d_depth, int64_t depth_n_bytes, const void* d_color,
                                                  int64_t color_n_bytes, vgx_projective_counts* counts);
/* HOST ONLY (no device, no context): the candidate block box [lo, hi] of a frame (both ends included).  Refuses what
 * vgx_depth_image_check refuses in the layout and the camera (byte counts aside) and the poses and reaches named above. */
VGX_API int vgx_tsdf_projective_box(const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                    const vgx_tsdf_config* cfg, const float T_G_C[7], float voxel_size, int32_t voxels_per_side,
                                    int32_t lo[3], int32_t hi[3]);

/* ---- LiDAR range images: a scan's points gathered into a spherical image, and its projective integration ---- */
/* The projective integrator above for a spinning LiDAR (voxblox's ProjectiveTsdfIntegrator is a LiDAR range-image integrator
 * [recalled]; not vendored: the rules are DEFINED here, what the kernels -- vgx_range_image.hip -- and
 * tests/range_image_ref.py both follow; f32 with one rounding per operation, no contraction, unless it says f64).  A scan
 * arrives as points, so the image is built first (vgx_range_image_build: two launches), then every voxel near a return looks
 * up ONE cell and updates itself (vgx_tsdf_integrate_range_image: one launch).  No atomic touches a voxel, nothing is sorted:
 * the same scans give the same layer, block order included, bit for bit on every run.
 *   angle rule  vgx_atan2_rule(y, x) below: NO library transcendental is part of a rule (atan2f of the device and of numpy do
 *               not agree bit for bit).  ax = |x|, ay = |y|, mx = fmaxf(ax, ay), mn = fminf(ax, ay); 0 unless mx > 0 [so
 *               (0, 0) gives 0]; q = mn / mx (one correctly rounded division, q in [0, 1]); s = q * q;
 *               p = C5; p = p * s + C4; ... ; p = p * s + C0 (Horner, a multiplication then an addition, each rounded);
 *               a = p * q; if ay > ax: a = PI_2 - a; if x < 0: a = PI - a; if y < 0: a = -a.  The coefficients (a fit of
 *               atan(q) / q in s over [0, 1]) and PI_2, PI are the hex floats below.  Its largest error against f64 atan2
 *               is at most VGX_ATAN2_RULE_MAX_ERROR (measured 1.92e-6 rad over 4e6 directions, seams and axes included:
 *               tests/test_range_image_cpu.py; the bar is 1 / 64 of the finest pitch accepted, 2 pi / 4096 / 64 = 2.4e-5).
 *               Inputs are finite; the results lie in [-PI, PI].
 *   model       vgx_lidar_model: width azimuth columns, height beam rows; azimuth_first_rad is the azimuth (atan2(y, x) in
 *               the sensor frame) of column 0's centre; columns advance towards growing azimuth, or -- azimuth_clockwise,
 *               as Ouster and Velodyne spin -- towards falling azimuth; elevation_first_rad / elevation_last_rad are the
 *               elevations (atan2(z, hypot(x, y))) of the centres of rows 0 and height - 1, the rows uniform between them
 *               (either may be the upper one).  Host constants, each rounded ONCE to f32 from f64:
 *               su = (azimuth_clockwise ? -1 : 1) * (double)width / 6.283185307179586,
 *               sv = (double)(height - 1) / ((double)elevation_last_rad - (double)elevation_first_rad).
 *               vgx_range_image_check refuses -- VGX_ERR_INVALID: NULL, an angle that is not finite, azimuth_first_rad
 *               outside [-PI, PI], the f32 constants (the column wrap below is ONE step), elevation_first_rad == elevation_last_rad with
 *               height > 1, an elevation outside (-pi/2, pi/2), width or height < 1; VGX_ERR_UNSUPPORTED: width > 4096,
 *               height > 256, width < 4, and height == 1 (a single beam has no pitch to take a row's extent from; no
 *               vertical aperture field is defined: refused).  Non-uniform rows, per-row azimuth offsets and
 *               single-row scanners: "LiDAR range images: beam tables" below.
 *   pixel       of a sensor-frame direction (x, y, z) with r = sqrtf(x x + y y + z z) (summed left to right), r > 0 and
 *               finite: rho = sqrtf(x x + y y), az = rule(y, x), el = rule(z, rho);
 *               uf = (az - azimuth_first_rad) * su, ua = uf + 0.5f, wrapped ONCE: if ua < 0: ua += (float)width, else if
 *               ua >= (float)width: ua -= (float)width; ui = floorf(ua) clamped to [0, width - 1] (the wrapped sum can
 *               round to width itself);  vf = (el - elevation_first_rad) * sv, va = vf + 0.5f; the row is accepted iff
 *               0 <= va < (float)height, vi = floorf(va).  Nearest pixel only.  A direction on the z axis has rho = 0,
 *               az = 0 and el = +-PI_2: outside every accepted model's rows unless a row reaches that far.
 *   image       vgx_range_image_build, from the points of a vgx_scan (any decode kind) or of a device array, indices in
 *               their order.  Point i is REJECTED BY RANGE unless r > 0 and r < +inf, else REJECTED BY ROW unless its row
 *               is accepted, else KEPT.  A cell holds the kept point of its pixel with the smallest r, of bit-equal r the
 *               smallest index [key = (u64)bits(r) << 32 | i under atomicMin: a positive float's bits order as the float
 *               does], whatever order the lanes run in: {range = r, rgba = the point's colour -- opaque white where the
 *               build is given no colours --, point_index = i}; an empty cell is {0, 0, -1}.  n_filled counts the cells
 *               that are not empty, n_collided = n_kept - n_filled.  Of the WINNING points the image keeps, in the sensor
 *               frame, max_range and per axis the smallest and largest coordinate (point_min / point_max) and the smallest
 *               and largest component of the unit direction (x / r, y / r, z / r: dir_min / dir_max): min / max and
 *               integer reductions, the order cannot show.  With no cell filled: max_range 0, the mins +inf, the maxs -inf.
 *               [The box of the returns "pulled in to max_ray_length_m and pushed out by the truncation" needs a
 *               vgx_tsdf_config; the build does not take one -- an image serves integrators of any configuration -- and
 *               keeps these raw extremes; vgx_tsdf_range_image_box finishes the box on the host.]
 *               The image owns what it needs: the scan handle may be decoded into again at once.  Two launches (scatter:
 *               one lane per point; resolve: one lane per cell) behind one memset, on the TSDF stream under the TSDF lock.
 *               counts != NULL: one read-back (the build's one host synchronisation); NULL: the build returns QUEUED and
 *               vgx_range_image_stats / _download / vgx_tsdf_integrate_range_image perform the read when they need it.
 *               n > 2^31 - 1 points: VGX_ERR_UNSUPPORTED.  n == 0: an image of empty cells.
 *   integrate   vgx_tsdf_integrate_range_image(integrator, T_G_S, image, counts).  Config fields READ and NOT read: as the
 *               depth-image integrator lists them above.  Per voxel: centre and the move into the sensor frame exactly as
 *               there (voxel, camera); r_v = sqrtf(x x + y y + z z), no update unless r_v > 0; the pixel by the rule
 *               above, no update outside the rows or where the cell is empty; r_s = the cell's range, sdf = r_s - r_v (the
 *               true distance along the ray).  gates, in this order: 1. r_s < min_ray_length_m: no update.  2. r_s >
 *               max_ray_length_m: an update only if allow_clear && voxel_carving_enabled && r_v + trunc <=
 *               max_ray_length_m, with sdf = max_ray_length_m - r_v, counted in n_cleared; the gates below are not asked.
 *               3. sdf < -trunc: no update.  4. sdf > trunc: an update only if voxel_carving_enabled, counted in n_carved.
 *               weight w = use_const_weight ? 1 : 1.0f / (r_s * r_s); if use_weight_dropoff && sdf < -voxel_size:
 *               w = fmaxf((w * (trunc + sdf)) / (trunc - voxel_size), 0).  No sparsity factor.  The colour is the cell's.
 *               update, blocks, counts (vgx_projective_counts): word for word as above.
 *   candidates  vgx_tsdf_range_image_box, on the host in f64: reach = min(max_ray_length_m, max_range) + trunc; refused
 *               (VGX_ERR_UNSUPPORTED) unless finite [an image with no cell filled: the box of the sensor origin alone].
 *               Per axis a of the sensor frame, over the winning points: a point pulled in to max_ray_length_m and pushed
 *               out by trunc along its own ray is u_a (min(r, max_ray) + trunc) with u its unit direction, and
 *               u_a min(r, max_ray) lies between 0 and both p_a and u_a max_ray: so
 *               hi_a = max(0, min(point_max_a, dir_max_a * max_ray)) + trunc * max(0, dir_max_a),
 *               lo_a = min(0, max(point_min_a, dir_min_a * max_ray)) + trunc * min(0, dir_min_a)  (the sensor origin is
 *               inside; an infinite max_ray_length_m pulls nothing in: point_max_a / point_min_a alone).  That box's eight corners are moved by T_G_S (as the library's transforms: uv = qv x P, uv += uv,
 *               cc = qv x uv, (P + qw uv + cc) + t); their axis-aligned box is widened on every side by
 *               reach * (pitch_az + pitch_el + 4 VGX_ATAN2_RULE_MAX_ERROR), pitch_az = 2 pi / width, pitch_el =
 *               |elevation_last_rad - elevation_first_rad| / (height - 1): a voxel's direction and its pixel's return each
 *               lie within half a pitch (and the rule's error) of the pixel centre in both angles, so the voxel is at most
 *               that angle off the return's ray, and at most reach times it away from the ray's point at its own range,
 *               which the unwidened box holds (r_v <= min(r_s, max_ray) + trunc by gates 2 to 4).  Then
 *               lo = floor(min / bs) - 1, hi = floor(max / bs) + 1 per axis, candidates in ascending (z, y, x), as above.
 *               The same caps: a pose that is not finite VGX_ERR_INVALID; beyond +-2^30 blocks, more than 2^24 candidates
 *               or a box the layer's block table cannot hold: VGX_ERR_UNSUPPORTED.
 *               [The kernel rejects whole blocks early: bounding sphere wholly beyond reach, or wholly above the upper
 *               row's cone or below the lower row's, the cones widened by half a pitch and the rule's error; a block that
 *               contains the sensor is never rejected.  That changes no value and no count.]
 * Streams and cost of the integration: as the depth-image integrator, without an upload -- the image is resident.  The
 * image is read until the frame has run; a build into the same handle is ordered behind it (one stream). */
#define VGX_ATAN2_RULE_MAX_ERROR 2.5e-6f
#define VGX_ATAN2_C0 0x1.fffd04p-1f
#define VGX_ATAN2_C1 -0x1.549b12p-2f
#define VGX_ATAN2_C2 0x1.8c5ed6p-3f
#define VGX_ATAN2_C3 -0x1.dce1aep-4f
#define VGX_ATAN2_C4 0x1.af48bap-5f
#define VGX_ATAN2_C5 -0x1.8001f8p-7f
#define VGX_ATAN2_PI_2 0x1.921fb6p+0f
#define VGX_ATAN2_PI 0x1.921fb6p+1f
typedef struct vgx_lidar_model {
  int32_t width, height;
  float azimuth_first_rad;
  int32_t azimuth_clockwise;
  float elevation_first_rad, elevation_last_rad;
} vgx_lidar_model;
typedef struct vgx_range_image_counts { /* of the image the handle holds */
  int64_t n_points, n_kept, n_filled, n_collided, n_rejected_range, n_rejected_rows;
  float max_range;
  float point_min[3], point_max[3], dir_min[3], dir_max[3];
  int32_t pad_;
} vgx_range_image_counts;
typedef struct vgx_range_image_s* vgx_range_image;
/* HOST ONLY: the rule itself, as the kernels evaluate it (built without contraction) */
VGX_API float vgx_atan2_rule(float y, float x);
/* HOST ONLY: VGX_OK, or why a model is refused */
VGX_API int vgx_range_image_check(const vgx_lidar_model* model);
/* HOST ONLY: the pixel rule; VGX_OK with *u, *v (v = -1: outside the rows), VGX_ERR_INVALID for NULL, a refused model or a
 * direction whose r is not positive and finite */
VGX_API int vgx_range_image_pixel(const vgx_lidar_model* model, float x, float y, float z, int32_t* u, int32_t* v);
VGX_API int vgx_range_image_create(vgx_ctx ctx, vgx_range_image* out);
VGX_API int vgx_range_image_destroy(vgx_range_image image);
VGX_API int vgx_range_image_build(vgx_range_image image, const vgx_lidar_model* model, vgx_scan scan,
                                  vgx_range_image_counts* counts /* NULL: queued, not waited for */);
/* the same from device arrays (f32 [n][3], u32 [n] bytes r g b a or NULL), ready with respect to the TSDF stream and read
 * until the build has run */
VGX_API int vgx_range_image_build_device(vgx_range_image image, const vgx_lidar_model* model, const void* d_points,
                                         const void* d_rgba, int64_t n, vgx_range_image_counts* counts);
/* the counts of the image held (waits for a queued build); the model it was built for in *model if not NULL */
VGX_API int vgx_range_image_stats(vgx_range_image image, vgx_range_image_counts* counts, vgx_lidar_model* model);
/* range [height][width] f32, rgba [height][width][4] bytes, point_index [height][width] i32; any may be NULL */
VGX_API int vgx_range_image_download(vgx_range_image image, float* range, uint8_t* rgba, int32_t* point_index);
VGX_API int vgx_tsdf_integrate_range_image(vgx_tsdf_integrator integrator, const float T_G_S[7], vgx_range_image image,
                                           vgx_projective_counts* counts /* NULL: queued, not waited for */);
/* HOST ONLY: the candidate block box [lo, hi] (both ends included) of an image with these counts */
VGX_API int vgx_tsdf_range_image_box(const vgx_lidar_model* model, const vgx_range_image_counts* image_counts,
                                     const vgx_tsdf_config* cfg, const float T_G_S[7], float voxel_size,
                                     int32_t voxels_per_side, int32_t lo[3], int32_t hi[3]);

/* ---- LiDAR range images: beam tables (non-uniform rows, per-row azimuth offsets, single-row scanners) ---- */
/* A second sensor model for the range image above: every row has an elevation of its own, boundaries derived
 * from its neighbours', and an azimuth offset.  The uniform model keeps its rule and its bits; this text is the definition
 * of the table rule, which vgx_range_image.hip and tests/beam_table_ref.py both follow.  Every call that takes the model
 * copies the two arrays before it returns.
 *   derived     host constants, each formed in f64 from the f32 inputs and rounded ONCE to f32.  su: the uniform model's.
 *               s_0 < ... < s_{H-1}: the elevations in ascending order (the table, or the table reversed);
 *               L = (double)row_half_extent_max_rad; mid_k = (s_k + s_{k+1}) * 0.5.  Interior boundaries:
 *               hi_k = min(mid_k, s_k + L), lo_{k+1} = max(mid_k, s_{k+1} - L) [L = +inf: the same f64, hence the same
 *               f32 -- no gap, no overlap].  Outer boundaries: lo_0 = s_0 - min(mid_0 - s_0, L),
 *               hi_{H-1} = s_{H-1} + min(s_{H-1} - mid_{H-2}, L).  H == 1: lo_0 = s_0 - L, hi_0 = s_0 + L.  After the
 *               rounding each boundary is clamped to [-VGX_ATAN2_PI_2, VGX_ATAN2_PI_2].
 *   check       vgx_range_image_check_beams refuses -- VGX_ERR_INVALID: a NULL model or elevation array, an angle that is
 *               not finite, |azimuth_first_rad| > PI, an elevation with |e| >= pi/2, a table that is not strictly
 *               monotone, a limit that is not > 0 (NaN included), an offset with |off| > VGX_ATAN2_PI_2, width or height
 *               < 1, height == 1 with an infinite limit, rounded boundaries that do not satisfy lo_k < hi_k and
 *               hi_k <= lo_{k+1} for every k; VGX_ERR_UNSUPPORTED: width > 4096, height > 256, width < 4.  A single row
 *               IS accepted when the limit is finite: the limit is its extent.
 *   pixel       of a direction with positive finite range; rho, az, el as above (vgx_atan2_rule).  Row: k* = the largest k
 *               with lo_k <= el, plain f32 compares; none, or !(el < hi_{k*}): outside the rows (above or below them, or
 *               in a gap between two rows the limit clipped).  vi = k* for an ascending table, H - 1 - k* for a
 *               descending one.  Column (defined only inside a row: it needs the row's offset):
 *               ua = ((az - azimuth_first_rad) - off_vi) * su + 0.5f, wrapped in TWO passes, each: if ua < 0:
 *               ua += (float)width, else if ua >= (float)width: ua -= (float)width  [|uf| <= 1.25 width: two passes always
 *               suffice, one does not]; ui = floorf(ua) clamped to [0, width - 1].  Nearest pixel only.
 *   image       vgx_range_image_build_beams / _beams_device: cells, keys, counts and extremes word for word as above;
 *               only the pixel rule differs.  n_rejected_rows includes directions in a gap.  One handle may hold a uniform
 *               image, then a table image, then a uniform one.  The image keeps the table on the device and uploads it
 *               (one copy on the TSDF stream, behind any frame that still reads the table held) only when it differs from
 *               the one held.  vgx_range_image_beams reports the table of the image held; vgx_range_image_stats fills its
 *               vgx_lidar_model with the shared fields and the table's FIRST and LAST elevation: a summary, not the model.
 *   integrate   vgx_tsdf_integrate_range_image, unchanged: the image knows which kind it holds.  Gates, weights, update,
 *               block order and counts as above.
 *   candidates  vgx_tsdf_range_image_box_beams: the uniform rule with pitch_el replaced by
 *               ext_max = max_k((double)hi_k - (double)lo_k) of the rounded boundaries: a voxel and its pixel's return lie
 *               in the same row and in the same column of that row's offset grid, at most one extent apart in each angle
 *               plus twice the rule's error.  [Early block reject: the cones of lo_0 and hi_{H-1}, widened by the rule's
 *               error; a cone that closes on the axis and the gaps between rows reject nothing.  No value, no count
 *               changes.] */
typedef struct vgx_lidar_beam_model {
  int32_t width, height;                /* columns; rows = beams                                   */
  float azimuth_first_rad;              /* as vgx_lidar_model                                      */
  int32_t azimuth_clockwise;            /* as vgx_lidar_model                                      */
  const float* row_elevation_rad;       /* [height], strictly ascending or strictly descending     */
  const float* row_azimuth_offset_rad;  /* [height] or NULL (zeros): added to azimuth_first_rad for that row */
  float row_half_extent_max_rad;        /* > 0; +inf: neighbouring rows meet halfway               */
} vgx_lidar_beam_model;
/* HOST ONLY: VGX_OK, or why a model is refused */
VGX_API int vgx_range_image_check_beams(const vgx_lidar_beam_model* model);
/* HOST ONLY: the pixel rule; VGX_OK with *u, *v (u = v = -1: outside the rows), VGX_ERR_INVALID for NULL, a refused model or
 * a direction whose r is not positive and finite */
VGX_API int vgx_range_image_pixel_beams(const vgx_lidar_beam_model* model, float x, float y, float z, int32_t* u, int32_t* v);
/* as vgx_range_image_build / _build_device: the same locks in the same order, the TSDF stream, queued without counts */
VGX_API int vgx_range_image_build_beams(vgx_range_image image, const vgx_lidar_beam_model* model, vgx_scan scan,
                                        vgx_range_image_counts* counts /* NULL: queued, not waited for */);
VGX_API int vgx_range_image_build_beams_device(vgx_range_image image, const vgx_lidar_beam_model* model, const void* d_points,
                                               const void* d_rgba, int64_t n, vgx_range_image_counts* counts);
/* the table the image held was built for: *is_table 0 (a uniform image; the other outputs are left alone) or 1, with
 * row_elevation [height], row_azimuth_offset [height] (zeros where the model gave NULL) and the limit; any may be NULL */
VGX_API int vgx_range_image_beams(vgx_range_image image, int32_t* is_table, float* row_elevation, float* row_azimuth_offset,
                                  float* row_half_extent_max_rad);
/* HOST ONLY: the candidate block box [lo, hi] (both ends included) of a table image with these counts */
VGX_API int vgx_tsdf_range_image_box_beams(const vgx_lidar_beam_model* model, const vgx_range_image_counts* image_counts,
                                           const vgx_tsdf_config* cfg, const float T_G_S[7], float voxel_size,
                                           int32_t voxels_per_side, int32_t lo[3], int32_t hi[3]);
/* HOST ONLY: dirs [height][width][3] f32, the unit direction through the centre of every pixel, computed in f64 and rounded
 * once: az = (azimuth_first_rad + off_row) + col / su with su in f64, el = row_elevation_rad[row], dir = (cos el cos az,
 * cos el sin az, sin el).  A sweep of exactly this sensor for the view renderer.  VGX_ERR_INVALID: NULL, a refused model */
VGX_API int vgx_view_rays_lidar_beams(const vgx_lidar_beam_model* model, float* dirs);

/* finishSubmap() hand-off without a host round trip: turns the active layer's blocks
 * into a (not yet finished) submap holding the raw TSDF layer and its TSDF sampling
 * grid; follow with vgx_submap_generate_esdf and vgx_submap_extract_voxel_points.  The
 * layer itself is left untouched (the mapper moves on to a new active submap). */
VGX_API int vgx_submap_from_tsdf_layer(vgx_ctx ctx, vgx_tsdf_layer layer, int32_t submap_id,
                                       vgx_submap* out);

/* Submaps that carry the TSDF voxels' colours (opt-in: a submap made by vgx_submap_create, vgx_submap_from_tsdf_layer or
 * vgx_map_file_load_submap has none, and every call on such a submap behaves as it always did).  Storage is one packed
 * uint32 per voxel (bytes r g b a, r lowest), as the layer keeps it: 4 B per voxel, spent only on submaps that asked.
 *   vgx_submap_from_tsdf_layer_colored  vgx_submap_from_tsdf_layer plus a device-to-device copy of the layer's rgba, in
 *                  the submap's block order, on the same stream and under the same locks; no host round trip.
 *   vgx_submap_set_colors  for host-built submaps (vgx_submap_create, or vgx_map_file_read_submap's tsdf_rgba): rgba
 *                  [n_blocks][vps^3][4] u8 in the order of vgx_submap_block_index; replaces colours already held
 *                  (staged through a fresh buffer: after any failure the old ones are whole).
 *                  VGX_ERR_INVALID, the submap unchanged: NULL rgba, a released raw TSDF layer.
 *   vgx_submap_has_colors  *has = 1 / 0.
 *   vgx_submap_download_colors  rgba [n_blocks][vps^3][4]; VGX_ERR_INVALID on a submap without colours.
 * vgx_submap_release_raw_layers frees the colours too (has_colors then reports 0).  What reads them: the projected map
 * and transformLayer (below), vgx_submap_generate_mesh_colored, vgx_submap_serialize_layer. */
VGX_API int vgx_submap_from_tsdf_layer_colored(vgx_ctx ctx, vgx_tsdf_layer layer, int32_t submap_id, vgx_submap* out);
VGX_API int vgx_submap_set_colors(vgx_submap submap, const uint8_t* rgba);
VGX_API int vgx_submap_has_colors(vgx_submap submap, int32_t* has);
VGX_API int vgx_submap_download_colors(vgx_submap submap, uint8_t* rgba);

/* The projected map: voxblox::mergeLayerAintoLayerB(submap TSDF layer, T_L_S, layer) applied to n submaps in ARRAY
 * order.  cblox::SubmapCollection::getProjectedMap() is this call on an empty layer (vgx_tsdf_layer_upload(layer, 0,
 * ...)) with the collection's submaps in ascending ID order and T_L_S = submap.getPose(); merging into a layer that
 * already holds data (an integrated one) behaves as repeated mergeLayerAintoLayerB calls would.  T_L_S [n][7] f32
 * {qw,qx,qy,qz, tx,ty,tz}.  *n_blocks_out (nullable): blocks in the layer afterwards.
 * Preconditions, each refused with VGX_ERR_INVALID (vgx_last_error says which) before the layer is touched: a submap
 * whose voxel_size or voxels_per_side differs from the layer's (voxblox would resample: not supported), whose raw TSDF
 * layer has been released (vgx_submap_release_raw_layers: keep the raw layers of submaps that will be projected), a
 * pose value that is not finite, |q.q - 1| > 1e-4, n < 0, NULL arrays with n > 0.  n = 0: VGX_OK, nothing changes.
 * Semantics (what the kernel and tests/projected_map_ref.py both follow):
 *   transform      T_S_L = T_L_S.inverse() once per submap in f32 (conjugate quaternion, translation -(q^-1 t)); the
 *                  sample point of layer voxel c is T_S_L * c (Eigen _transformVector, then + t), c the voxel centre
 *                  origin + (idx + 0.5) * voxel_size.
 *   interpolation  Interpolator<TsdfVoxel>::getVoxel(p, &v, true) [recalled], as the isosurface points use it: all 8
 *                  neighbours allocated with weight > 0, distance and weight interpolated trilinearly.
 *   coverage       submap s contributes to layer block b iff at least one voxel centre of b interpolates in s.  Then b
 *                  is allocated if absent (new voxels d = 0, w = 0, rgba = 0) and EVERY voxel of b is merged, one that
 *                  did not interpolate as the default voxel (0, 0) -- which is not a no-op: (0*0 + d*w) / w need not be
 *                  d.  [recalled] voxblox allocates the intermediate layer's blocks from the transformed extent of each
 *                  input block and drops blocks that received no data; this rule is what that yields wherever that
 *                  allocation covers every block with an interpolable centre.
 *   merge          mergeVoxelAIntoVoxelB [recalled] (A: the submap's voxel, B: the layer's): w' = wA + wB; if w' > 0,
 *                  d = (dA*wA + dB*wB) / w' and w = w' (f32, that association, no contraction); else unchanged.  No
 *                  weight cap.
 *   colour         a submap without colours leaves rgba untouched, exactly as before (voxblox blends it: a submap has to
 *                  carry colours for that, vgx_submap_from_tsdf_layer_colored / vgx_submap_set_colors).  A submap with
 *                  colours also merges colour, all [recalled]:
 *                    colour of A, interpolated voxel: Interpolator<TsdfVoxel>::interpVoxel per channel -- the 8
 *                      neighbours' channel bytes widened to f32, in the neighbour order of the interpolation (k = 0..7:
 *                      x offset = bit 2, y = bit 1, z = bit 0), through the same trilinear form with the same dl as
 *                      distance and weight.  voxblox assigns that float to a uint8_t member; here the value is clamped
 *                      to [0, 255] first, then truncated toward zero: a stated definition for the few-ulp overshoots
 *                      that the C++ cast leaves undefined.
 *                    colour of A, voxel that did not interpolate: the default voxel's (0, 0, 0, 0), w = 0.
 *                    merge: where the rule above updates the voxel (w' = wA + wB > 0) the colour becomes
 *                      Color::blendTwoColors(cB, wB, cA, wA) with the PRE-merge weights (per channel
 *                      round(b * (wB / w') + a * (wA / w')), f32, as the integrators and the MERGE action blend);
 *                      otherwise it is unchanged.
 *                  Array order is the merge order for colour as for distance; submaps with and without colours may be
 *                  mixed in one call.  Newly allocated blocks start at rgba 0.
 * Runs on the context's TSDF stream behind the registration stream (where submap layers are produced); takes the TSDF
 * lock, then the registration lock; returns once the sources have been read, so the caller may destroy a submap or
 * release its raw layers right after.  Room for every candidate block is reserved first: VGX_ERR_NOMEM then, before
 * any voxel is touched.  Values do not depend on scheduling; the slots of newly allocated blocks (their order in
 * vgx_tsdf_layer_download) may, as after a scan. */
VGX_API int vgx_tsdf_layer_merge_submaps(vgx_tsdf_layer layer, int32_t n, const vgx_submap* submaps, const float* T_L_S, int64_t* n_blocks_out);

/* voxblox::transformLayer(submap TSDF layer, T_L_S, layer) [recalled] into an EMPTY layer: the resampling behind
 * VoxgraphSubmap::transformSubmap (voxgraph_submap.cpp:38-59), which MapEvaluation::evaluate applies to the ground
 * truth once it is aligned (map_evaluation.cpp:86).  transformSubmap on the device is this call, then
 * vgx_submap_from_tsdf_layer and vgx_submap_generate_esdf.  T_L_S {qw,qx,qy,qz, tx,ty,tz} f32.  *n_blocks_out
 * (nullable): blocks in the layer.  The rules are those of vgx_tsdf_layer_merge_submaps with n = 1 -- the f32 inverse
 * pose, the voxel centres, the interpolation and the coverage rule (a block is kept iff one of its voxel centres
 * interpolates) -- except that the voxel is COPIED, not merged: an interpolated voxel gets {d, w} as interpolated,
 * every other voxel of a kept block stays (0, 0).  That is not a merge into an empty layer: (d*w + 0*0) / w need not
 * round back to d.  A submap without colours leaves rgba untouched; a submap with colours stores an interpolated
 * voxel's interpolated colour (the colour rule of vgx_tsdf_layer_merge_submaps) and (0, 0, 0, 0) on every other voxel
 * of a kept block.  [recalled] some voxblox versions fall back to the nearest voxel where trilinear interpolation
 * fails; the pinned version could not be checked: here a voxel that does not interpolate is not written (DESIGN.md 9,
 * "Known gaps").
 * Preconditions, each refused with VGX_ERR_INVALID before anything is written: NULL handles or pose, a layer that is not
 * empty, a voxel_size or voxels_per_side that differs from the layer's, a released raw TSDF layer, a pose that is not
 * finite or whose |q.q - 1| > 1e-4.  Streams, locks and lifetimes: those of vgx_tsdf_layer_merge_submaps. */
VGX_API int vgx_tsdf_layer_transform_submap(vgx_tsdf_layer layer, vgx_submap submap, const float T_L_S[7],
                                            int64_t* n_blocks_out);

/* The combined mesh: voxblox::MeshIntegrator<TsdfVoxel>::generateMesh(false, false) [recalled] over a whole TSDF layer.
 * cblox SubmapMesher::generateCombinedMesh (SubmapVisuals::publishCombinedMesh / saveCombinedMesh) is the projected map
 * (vgx_tsdf_layer_merge_submaps) followed by this call on the layer; the active-submap mesh and MapEvaluation's
 * ground-truth mesh are the same call on one layer (vgx_submap_generate_mesh reads a finished submap's raw layer, in the
 * submap frame).  Everything about voxblox here is [recalled]: voxblox is not vendored.
 * Semantics (what the kernels, vgx_mesh.hip, and tests/mesh_ref.py both follow):
 *   cubes          block b owns the cube whose low corner is its voxel (x,y,z), every x,y,z in [0, vps)
 *                  (MeshIntegrator::extractBlockMesh).  Its 8 corners are that voxel + cube_index_offsets_ in the order
 *                  (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); a corner outside b is read from the
 *                  neighbouring block (+x, +y, +z and their combinations).  A cube is meshed only if every corner exists
 *                  and has weight > min_weight (utils::getSdfIfValid); a missing neighbour block skips the cube.
 *   visiting order (fixes the triangle order within a block) 1. the interior cubes x,y,z < vps-1, x outermost, z
 *                  innermost; 2. the max-X plane x = vps-1 (z outer, y inner, both in [0, vps)); 3. the max-Y plane
 *                  y = vps-1 (z outer, x inner, x < vps-1); 4. the max-Z plane z = vps-1 (y outer, x inner, x,y < vps-1).
 *   coordinates    corner i = coords + offset_i * voxel_size, coords the low voxel's centre origin + (idx + 0.5f) *
 *                  voxel_size, origin = block_index * block_size (f32; the rule of vgx_tsdf_layer_merge_submaps).  A
 *                  corner is NOT the neighbour voxel's own centre recomputed: the two round differently.
 *   per cube       (MarchingCubes::meshCube) configuration bit i set when sdf_i < 0; edges kEdgeIndexPairs {0,1} {1,2}
 *                  {2,3} {3,0} {4,5} {5,6} {6,7} {7,4} {0,4} {1,5} {2,6} {3,7} in that direction; the vertex on edge
 *                  (a, b) is pa + t * (pb - pa), t = sa / (sa - sb), when |sa - sb| >= 1e-6f, else 0.5f * (pa + pb)
 *                  (f32, that association, no contraction).  Each triple (e0, e1, e2) of the classic Lorensen / Bourke
 *                  table (voxgraph_amd/csrc/vgx_mc_tables.h) is emitted as the vertices e2, e1, e0; its normal is
 *                  (p1 - p0) x (p2 - p0) over the emitted order (Eigen's cross-product formulas) divided by
 *                  sqrt((x*x + y*y) + z*z), the zero vector kept when that sum is 0 (Eigen normalized()).
 *   triangle soup  edge direction is not shared between cubes: edges 2, 3, 6, 7 run high to low, so the up to four cubes
 *                  around one grid edge may give bitwise-different copies of its vertex -- voxblox's soup, reproduced.
 *                  The isosurface points (vgx_submap_extract_isosurface_points) interpolate low to high from independently
 *                  computed centres and stay as they are: the two agree to the last bits only.
 *   output         one entry per allocated TSDF block (voxblox's MeshLayer: one mesh per block, possibly empty), in
 *                  ascending (x, y, z) block-index order whatever the layer's slot order.  Block k owns the triangles
 *                  [first[k], first[k+1]); vertices [T][3][3] f32 in the emitted order (voxblox's indices are implicitly
 *                  0..3n-1 per block); normals [T][3] f32, one per triangle (voxblox stores it three times).
 *   colour         these two calls make no colour (MeshIntegratorConfig::use_color = false); the _colored forms below
 *                  are use_color = true.
 *   deviations     only_mesh_updated_blocks / clear_updated_flag are not supported (every caller passes false, false).
 * A mesh handle is reused from call to call (the mapper re-meshes after every submap): its device buffers grow on demand;
 * one call at a time per handle.  Refused with VGX_ERR_INVALID before anything is written: NULL handles, a min_weight that
 * is negative or not finite, a source and mesh of different contexts, a submap whose raw TSDF layer was released.  An
 * empty layer gives VGX_OK and 0 blocks.  Out of device memory: VGX_ERR_NOMEM, and the handle then holds no mesh (stats
 * report 0).  The layer source runs on the context's TSDF stream behind the scans and merges already queued, under the
 * TSDF lock and then the registration lock (so a projected map can be meshed right after it is built); the submap source
 * runs on the registration stream under the registration lock.  Both return with the mesh complete; values and their
 * order do not depend on scheduling. */
typedef struct vgx_mesh_s* vgx_mesh;
typedef struct vgx_mesh_config {
  float min_weight; /* 1e-4 (MeshIntegratorConfig [recalled]) */
} vgx_mesh_config;
VGX_API void vgx_mesh_config_default(vgx_mesh_config* cfg);
VGX_API int vgx_mesh_create(vgx_ctx ctx, vgx_mesh* out);
VGX_API int vgx_mesh_destroy(vgx_mesh mesh);
/* cfg == NULL: the defaults */
VGX_API int vgx_tsdf_layer_generate_mesh(vgx_tsdf_layer layer, const vgx_mesh_config* cfg, vgx_mesh mesh);
VGX_API int vgx_submap_generate_mesh(vgx_submap submap, const vgx_mesh_config* cfg, vgx_mesh mesh);
/* MeshIntegratorConfig::use_color = true: the generator above, unchanged, then MeshIntegrator::updateMeshColor
 * [recalled] as one streaming kernel over the soup -- same stream, same locks, no further host synchronisation.  Vertices,
 * normals, first and block_index are those of the plain call; the mesh additionally holds one colour per soup vertex
 * ([T][3][4] u8, vgx_mesh_download_vertex_colors).  The submap form needs a submap with colours (VGX_ERR_INVALID
 * otherwise, the handle keeping what it held); the layer form reads the layer's rgba.
 * Rule for vertex p of a triangle of block b (origin = block_index * block_size, f32): the voxel index in b is
 * floorf((p[a] - origin[a]) * voxel_size_inv + 1e-6f) per axis; if all three lie in [0, vps) that voxel is taken.
 * Otherwise (a vertex on one of b's max planes) the block is floorf(p[a] * block_size_inv + 1e-6f) and the index the
 * formula above against that block's origin, clamped to [0, vps - 1] (the nearest-voxel rule of vgx_submap_query).  The
 * vertex gets the voxel's colour byte for byte if its weight >= min_weight (utils::getColorIfValid); else it keeps the
 * default (0, 0, 0, 0), as does a vertex whose block is absent (voxblox would dereference null there).  A vertex lies on
 * an edge between two corners that passed weight > min_weight, so the default is reached only through rounding. */
VGX_API int vgx_tsdf_layer_generate_mesh_colored(vgx_tsdf_layer layer, const vgx_mesh_config* cfg, vgx_mesh mesh);
VGX_API int vgx_submap_generate_mesh_colored(vgx_submap submap, const vgx_mesh_config* cfg, vgx_mesh mesh);
VGX_API int vgx_mesh_stats(vgx_mesh mesh, int32_t* n_blocks, int64_t* n_triangles);
/* block_index [nb][3], first [nb+1], vertices [T][3][3], normals [T][3]; any may be NULL */
VGX_API int vgx_mesh_download(vgx_mesh mesh, int32_t* block_index, int64_t* first, float* vertices, float* normals);
/* Host code: binary_little_endian PLY of the triangle soup -- vertex x y z nx ny nz (float; the triangle's normal on
 * each of its three vertices; then red green blue alpha (uchar) when the mesh has colours: the vertex's own on a
 * per-vertex mesh, else its triangle's), face `list uchar int vertex_indices` = (3t, 3t+1, 3t+2).  A stated format, not
 * byte parity with voxblox's outputMeshLayerAsPly. */
VGX_API int vgx_mesh_write_ply(vgx_mesh mesh, const char* path);
/* The triangle table the kernels use (voxgraph_amd/csrc/vgx_mc_tables.h): row c = the triangles of configuration c as
 * edge triples, -1 terminated.  Host only (no device needed). */
VGX_API int vgx_mesh_triangle_table(int8_t out[256][16]);

/* The separated mesh: cblox SubmapMesher::generateSeparatedMesh [recalled] (SubmapVisuals::publishSeparatedMesh /
 * saveSeparatedMesh, submap_visuals.cpp:67-97) over n finished submaps, into one mesh handle.  cblox meshes each submap
 * in its own frame (generateMesh(false, false)), colours it (colorMeshLayer), transforms it (transformMeshLayer(T_M_S))
 * and appends it to one MeshLayer keyed by the submap-frame block index.  T_M_S [n][7] f32 {qw,qx,qy,qz, tx,ty,tz} (the
 * collection's submaps in ascending ID order at getPose(), as the projected map takes them); rgba [n][4] u8.
 * Rules (what the kernels, vgx_mesh.hip, and tests/separated_mesh_ref.py all follow):
 *   triangles      per submap exactly those of vgx_submap_generate_mesh on that submap: the same cubes, visiting order,
 *                  f32 edge interpolation, and the normal computed in the submap frame.  Only then each vertex becomes
 *                  transform_point(q, t, p) (Eigen _transformVector, then + t; no contraction) and each normal the same
 *                  rotation without t, not renormalised.
 *   colour         every triangle of submap s gets rgba[s], stored once per triangle ([T][4] u8; voxblox stores it on each
 *                  of the three vertices).  The colour is an input: the rule that picks it is not pinned (voxgraph's own
 *                  per-submap rule for its active-submap mesh is rainbowColorMap(id / 20) [recalled]; the Python and C++
 *                  layers default to it).
 *   combination    every allocated block of every submap, empty mesh or not, makes or joins one output entry keyed by its
 *                  submap-frame block index; entries in ascending (x, y, z) order (block_index has no duplicates).
 *                  Within an entry the submaps' triangles come in ARRAY order, each submap's in its own block order.
 *                  first [nb+1], vertices and normals: the layout of vgx_tsdf_layer_generate_mesh.
 *   handle         afterwards vgx_mesh_has_colors reports 1; vgx_tsdf_layer_generate_mesh and vgx_submap_generate_mesh
 *                  clear it and change in nothing else.  vgx_mesh_download_colors on a mesh without colours:
 *                  VGX_ERR_INVALID.  vgx_mesh_download and vgx_mesh_stats are unchanged.
 * Refused with VGX_ERR_INVALID before anything is launched (vgx_last_error says which): NULL ctx or mesh, a mesh of
 * another context, n < 0, NULL arrays with n > 0, a NULL submap or one of another context, a released raw TSDF layer,
 * voxel_size or voxels_per_side that differ across the submaps, a pose that is not finite or whose |q.q - 1| > 1e-4, a
 * min_weight that is negative or not finite.  VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16, a union block box
 * whose cell count x n does not fit a 64-bit key, more than 2^31 - 1 blocks in all.  n = 0 (or only empty submaps):
 * VGX_OK, 0 blocks and a mesh with colours.  Out of device memory: VGX_ERR_NOMEM, and the handle then holds no mesh.
 * Streams and locks: those of vgx_submap_generate_mesh (the registration stream, under the registration lock).  One pass
 * over all n submaps: a fixed number of launches and two host synchronisations whatever n; returns with the mesh
 * complete; values and their order do not depend on scheduling.
 * vgx_mesh_write_ply adds `property uchar red / green / blue / alpha` after the normals when the mesh has colours (the
 * triangle's colour on each of its vertices); a mesh without colours gives the file it always gave. */
VGX_API int vgx_submaps_generate_separated_mesh(vgx_ctx ctx, int32_t n, const vgx_submap* submaps, const float* T_M_S,
                                                const uint8_t* rgba, const vgx_mesh_config* cfg, vgx_mesh mesh);
/* *has = 1 when the mesh carries colours (a separated mesh, a _colored mesh), else 0 */
VGX_API int vgx_mesh_has_colors(vgx_mesh mesh, int32_t* has);
/* *layout = which colours: none, one per triangle (a separated mesh), one per soup vertex (a _colored mesh) */
#define VGX_MESH_COLORS_NONE 0
#define VGX_MESH_COLORS_PER_TRIANGLE 1
#define VGX_MESH_COLORS_PER_VERTEX 2
VGX_API int vgx_mesh_color_layout(vgx_mesh mesh, int32_t* layout);
/* rgba [T][4]: one colour per triangle.  VGX_ERR_INVALID on a per-vertex mesh (the size differs) */
VGX_API int vgx_mesh_download_colors(vgx_mesh mesh, uint8_t* rgba);
/* rgba [T][3][4]: one colour per soup vertex.  VGX_ERR_INVALID unless the layout is per vertex */
VGX_API int vgx_mesh_download_vertex_colors(vgx_mesh mesh, uint8_t* rgba);

/* The connected mesh: voxblox MeshLayer::getConnectedMesh / createConnectedMesh [recalled] over the triangle soup a
 * vgx_mesh holds -- what voxblox::outputMeshLayerAsPly writes (SubmapVisuals::saveCombinedMesh / saveSeparatedMesh,
 * submap_visuals.cpp:89-107) and what VoxgraphSubmap::findIsosurfaceVertices asks for at 0.5 * voxel_size.  Vertices
 * that fall into the same cell of a grid of pitch `approximate_vertex_proximity_threshold` become one vertex, and the
 * triangles an index list.  The source is any vgx_mesh that holds a mesh (of a layer, of a submap, a separated mesh); it
 * is not changed.  Everything about voxblox here is [recalled]: voxblox is not vendored.
 * Rules (what the kernels, vgx_connect.hip, and tests/connected_mesh_ref.py all follow):
 *   soup order     soup vertex j = 3 t + c is corner c of triangle t in the order vgx_mesh_download returns: blocks in
 *                  ascending (x, y, z) block index, then the block's triangles, then the three corners.  DEVIATION:
 *                  voxblox walks its block meshes in hash-map order, which is not defined; ascending block order is this
 *                  library's stated order (the "output" rule of vgx_tsdf_layer_generate_mesh).  It decides which copy of
 *                  a welded vertex is the "first".
 *   key            inv = 1.0 / (double)threshold, the threshold an f32 (voxblox's FloatingPoint; its default 1e-10f).
 *                  Per coordinate k = (int64) round((double)v * inv): one f64 multiply, std::round (halves away from
 *                  zero), so -0.0 and +0.0 share key 0.  The key is the three int64 together, compared exactly (192
 *                  bits): a hash of them finds the slot, it never decides equality.
 *   vertices       a key's vertex is its FIRST soup vertex (smallest j): its three floats copied bit for bit, the
 *                  normal of that soup vertex's triangle j / 3 (voxblox stores the triangle normal on each corner) and,
 *                  when the source has colours, the colour of triangle j / 3 -- or, on a per-vertex mesh, soup vertex
 *                  j's own colour.  Unique vertices are numbered in order of first occurrence (ascending j).
 *   indices        indices[j] = the number of the unique vertex of key(j): [T][3] u32, triangle order unchanged.
 *                  Triangles whose corners weld together are kept (voxblox keeps them).  Blocks without triangles
 *                  contribute nothing.
 * The output handle is reused from call to call: its device buffers grow on demand; one call at a time per handle.
 * Refused with VGX_ERR_INVALID before anything is launched: NULL handles, handles of different contexts, a threshold that
 * is not finite or not > 0, a source handle that holds no mesh because its last generating call failed.
 * VGX_ERR_UNSUPPORTED: 3 T >= 2^32; a vertex with a coordinate that is not finite or with |v * inv| >= 2^62 (the int64
 * cast is undefined there; found by a device flag after the first passes, and the output handle then holds no mesh: stats
 * report 0).  Out of device memory: VGX_ERR_NOMEM, and the output handle then holds no mesh.  A source with 0 triangles:
 * VGX_OK, 0 vertices, 0 triangles.  has_colors follows the source.
 * Runs on the registration stream under the registration lock (a vgx_mesh is complete when its generating call returns,
 * whichever stream made it); returns with the connected mesh complete.  Two memsets, three kernels and one scan whatever
 * the size, and two host synchronisations (the vertex count and the range flag in one; the end).  Values and order do not
 * depend on scheduling: the only atomics are integer ones whose final value is order-independent (the claim of an empty
 * slot, a minimum, the OR of the range flag). */
typedef struct vgx_connected_mesh_s* vgx_connected_mesh;
VGX_API int vgx_connected_mesh_create(vgx_ctx ctx, vgx_connected_mesh* out);
VGX_API int vgx_connected_mesh_destroy(vgx_connected_mesh cm);
VGX_API int vgx_mesh_connect(vgx_mesh mesh, float approximate_vertex_proximity_threshold, vgx_connected_mesh out);
/* any pointer may be NULL */
VGX_API int vgx_connected_mesh_stats(vgx_connected_mesh cm, int64_t* n_vertices, int64_t* n_triangles, int32_t* has_colors);
/* vertices [V][3], normals [V][3], rgba [V][4], indices [T][3]; any may be NULL.  rgba on a mesh without colours:
 * VGX_ERR_INVALID. */
VGX_API int vgx_connected_mesh_download(vgx_connected_mesh cm, float* vertices, float* normals, uint8_t* rgba,
                                        uint32_t* indices);
/* Host code: binary_little_endian PLY -- element vertex V: x y z nx ny nz (float), then red green blue alpha (uchar) when
 * the mesh has colours; element face T: `list uchar int vertex_indices`.  VGX_ERR_UNSUPPORTED when V >= 2^31.  A stated
 * format, not byte parity with voxblox's outputMeshLayerAsPly.  vgx_mesh_write_ply (the soup) is unchanged. */
VGX_API int vgx_connected_mesh_write_ply(vgx_connected_mesh cm, const char* path);

/* Mesh markers: voxblox_ros fillMarkerWithMesh [recalled] over the triangle soup a vgx_mesh holds -- marker.points and
 * marker.colors of the visualization_msgs/Marker (TRIANGLE_LIST) that SubmapVisuals::publishCombinedMesh
 * (submap_visuals.cpp:78-87, ColorMode::kNormals), publishSeparatedMesh (:68-76) and publishMesh (:45-66, after cblox
 * colorMeshLayer; both with the default kLambertColor, submap_visuals.h:25-29) publish, with mesh_opacity_ written into
 * every alpha (:36-39).  The source is any vgx_mesh that holds a mesh (of a layer, of a submap, a separated mesh); it is
 * not changed.  Everything about voxblox_ros here is [recalled]: it is not vendored.
 * Rules (what the kernel, vgx_marker.hip, and tests/mesh_marker_ref.py both follow):
 *   order          marker point j = 3 t + c is soup vertex j in the order of vgx_mesh_download (corner c of triangle t);
 *                  blocks without triangles contribute nothing; n_points = 3 T.
 *   points         [n][3] f64: each f32 coordinate widened (exact).
 *   colors         [n][4] f32 r g b a.  a = opacity on every vertex, whatever the mode.
 *   vertex colour  the colour of its triangle (vgx_mesh_download_colors) or, on a per-vertex mesh, its own
 *                  (vgx_mesh_download_vertex_colors: COLOR and LAMBERT_COLOR shade every vertex apart), or
 *                  constant_rgba when use_constant_color is set (cblox colorMeshLayer before the colouring).  c8(k) =
 *                  (float)((double)k / 255.0) of a channel byte k: a 256-entry f32 table built on the host, so no
 *                  device division decides a bit.
 *   GRAY           r = g = b = 0.5f.
 *   COLOR          (c8(r), c8(g), c8(b)).
 *   NORMALS        per channel (float)((double)n * 0.5 + 0.5), n the triangle normal's component (the product is exact in
 *                  f64, so contraction cannot change it).
 *   LAMBERT_COLOR  all f32, no contraction.  L1 = (0.8f, -0.2f, 0.7f), L2 = (-0.5f, 0.2f, 0.2f), each divided component
 *                  by component by sqrtf((x*x + y*y) + z*z) (on the host, once).  d_i = (n.x*Li.x + n.y*Li.y) + n.z*Li.z,
 *                  then d_i = (d_i < 0.0f) ? 0.0f : d_i.  Per channel with c = c8(.): v = (d1*c + d2*c) + 0.2f, and the
 *                  output is (1.0f < v) ? 1.0f : v.
 *   LAMBERT        LAMBERT_COLOR with the colour (127, 127, 127).
 *   HEIGHT         per vertex, from its own z: t = (float)(((double)z + 1.0) / 11.0), t = (t < 0) ? 0 : t, then
 *                  t = (1.0f < t) ? 1.0f : t; the bytes of rainbowColorMap((double)t) (the map of the separated mesh's
 *                  default colours), each channel through c8.  A z that is not a number takes the map's default case
 *                  (255, 127, 127).
 *   degenerate     a zero normal (a degenerate triangle keeps it) goes through the same formulas: NORMALS gives 0.5,
 *   triangles      LAMBERT the ambient 0.2.
 * The marker handle is reused from call to call: its device buffers grow on demand; one call at a time per handle.
 * Refused with VGX_ERR_INVALID before anything is written, the handle keeping what it held (vgx_last_error says which):
 * NULL handles, handles of different contexts, an unknown color_mode, an opacity that is not finite, a source handle that
 * holds no mesh because its last generating call failed, COLOR or LAMBERT_COLOR on a mesh without colours and without
 * use_constant_color (voxblox CHECKs hasColors() there).  VGX_ERR_UNSUPPORTED (the handle keeps what it held, too):
 * 3 T >= 2^32, a ROS array length being a u32.  Out of device memory: VGX_ERR_NOMEM, and the handle then holds nothing
 * (stats report 0 points).  A source with 0 triangles: VGX_OK and 0 points.  A NULL cfg means the defaults.
 * Runs on the registration stream under the registration lock (a vgx_mesh is complete when its generating call returns,
 * whichever stream made it); returns with the marker complete.  One kernel whatever the size (and, on a handle's first
 * use, the 1 KiB copy of the c8 table), one host synchronisation; no atomics, no scan: T is known on the host.  Out of
 * scope: voxblox_msgs/Mesh (generateVoxbloxMeshMsg), ROS message types and the serialisation of the header fields, the
 * other markers voxgraph publishes (boxes, pose-graph edges, the cost-function visuals), markers from a connected mesh. */
#define VGX_MARKER_COLOR 0 /* voxblox ColorMode, in its order [recalled] */
#define VGX_MARKER_HEIGHT 1
#define VGX_MARKER_NORMALS 2
#define VGX_MARKER_GRAY 3
#define VGX_MARKER_LAMBERT 4
#define VGX_MARKER_LAMBERT_COLOR 5
typedef struct vgx_mesh_marker_config {
  int32_t color_mode;         /* VGX_MARKER_LAMBERT_COLOR (submap_visuals.h:28-29) */
  float opacity;              /* 1.0f: SubmapVisuals::mesh_opacity_ */
  int32_t use_constant_color; /* 0; 1 = cblox colorMeshLayer(constant_rgba) before colouring */
  uint8_t constant_rgba[4];   /* 0 0 0 0 */
} vgx_mesh_marker_config;
VGX_API void vgx_mesh_marker_config_default(vgx_mesh_marker_config* cfg);
typedef struct vgx_mesh_marker_s* vgx_mesh_marker;
VGX_API int vgx_mesh_marker_create(vgx_ctx ctx, vgx_mesh_marker* out);
VGX_API int vgx_mesh_marker_destroy(vgx_mesh_marker marker);
/* cfg NULL: the defaults */
VGX_API int vgx_mesh_fill_marker(vgx_mesh mesh, const vgx_mesh_marker_config* cfg, vgx_mesh_marker out);
/* either pointer may be NULL; color_mode: that of the last accepted fill */
VGX_API int vgx_mesh_marker_stats(vgx_mesh_marker marker, int64_t* n_points, int32_t* color_mode);
/* points [n][3] f64, colors [n][4] f32; either may be NULL */
VGX_API int vgx_mesh_marker_download(vgx_mesh_marker marker, double* points, float* colors);
/* the device arrays of the marker held now (NULL when it holds 0 points); valid until the next fill or destroy */
VGX_API int vgx_mesh_marker_device_pointers(vgx_mesh_marker marker, const double** points, const float** colors);

/* ---- Map evaluation: voxblox::utils::evaluateLayersRmse ------------------- */
/* MapEvaluation::evaluate (map_evaluation.cpp:59-114) scores a map against a ground truth: projected map
 * (vgx_tsdf_layer_merge_submaps), finishSubmap() of both (vgx_submap_from_tsdf_layer, vgx_submap_generate_esdf,
 * vgx_submap_extract_voxel_points), alignment (REG), transformSubmap (vgx_tsdf_layer_transform_submap) and then
 * evaluateLayersRmse(gt ESDF, test ESDF, kIgnoreErrorBehindTestSurface, &details, &error_layer), which is this call.
 * gt and test are finished submaps of one context; `layer` picks their raw ESDF or raw TSDF layer.
 * Rules (what the kernels, vgx_eval.hip, and tests/map_eval_ref.py both follow; [recalled]: voxblox owns them):
 *   blocks    matched by index through each submap's dense block table.  A test block without a gt block of the same
 *             index adds vps^3 to num_non_overlapping_voxels; so does a gt block without a test block.
 *   observed  ESDF: observed != 0; TSDF: weight > 1e-6f [recalled].
 *   voxel     unobserved in either layer: non-overlapping.  Else, if the mode ignores the test side (IGNORE_BEHIND_TEST,
 *             _ALL) and d_test < 0, or the gt side (IGNORE_BEHIND_GT, _ALL) and d_gt < 0: ignored (and overlapping).
 *             Else evaluated (and overlapping): e = d_test - d_gt in f32; the sum gains (double)(e*e), the product in f32;
 *             max_error = max |e| (from 0).
 *   results   rmse = (float)sqrt(total_squared_error / num_evaluated_voxels), 0 when nothing was evaluated (voxblox
 *             divides by zero there).  min_error: voxblox starts it at 0 and only takes min(), so it reports 0 [recalled];
 *             that is what is reported.  min_abs_error is the true minimum of |e| (0 when nothing was evaluated).
 *   sum order (fixed, so the f64 sum is bit-identical run to run) per test block: voxel v = 4 (t + T k) + j is summed
 *             by thread t (T = min(256, vps^3 / 4) threads), k outer and j inner, from 0.0; the threads of a wave are
 *             folded by a __shfl_down tree (offsets 32, 16, .., 1; lane 0 keeps the result), the waves in order
 *             ((w0 + w1) + w2) + ...  Over the test blocks, in slot order: block b is summed by thread b mod 1024 of one
 *             1024-thread workgroup, in ascending b from 0.0; then the same wave tree and waves in order.
 *   error     one error block per test block that has a gt counterpart, in test-slot order (*n_error_blocks of them):
 *   layer     error_block_index [m][3], and per voxel error_distance = e, error_set = 1 for an evaluated voxel, (0, 0)
 *             for every other -- voxblox's setVoxelSdf / setVoxelWeight(1) into an ESDF or TSDF error layer.  The
 *             three arrays are sized for n_test blocks (vps^3 entries per block); any may be NULL.
 * Refused with VGX_ERR_INVALID before anything is written: NULL handles or details, submaps of different contexts, a
 * voxel_size or vps mismatch (the reference's CHECK_EQ), a layer or mode value out of range, a layer the submap no longer
 * holds in raw form (released, or an ESDF never generated).  Runs on the context's registration stream under its lock,
 * as vgx_submap_generate_esdf (which produces the ESDF layers read here) does; returns with the results on the host:
 * one D2H of the details, plus the error layer when asked for. */
#define VGX_EVAL_ALL_VOXELS 0 /* voxblox VoxelEvaluationMode order [recalled] */
#define VGX_EVAL_IGNORE_BEHIND_TEST 1
#define VGX_EVAL_IGNORE_BEHIND_GT 2
#define VGX_EVAL_IGNORE_BEHIND_ALL 3
#define VGX_EVAL_LAYER_ESDF 0
#define VGX_EVAL_LAYER_TSDF 1
typedef struct vgx_voxel_evaluation_details {
  float rmse, max_error, min_error; /* as voxblox stores them (f32)                  */
  double total_squared_error;       /* the f64 sum rmse comes from                    */
  float min_abs_error;              /* the true minimum; see min_error above          */
  int64_t num_evaluated_voxels, num_ignored_voxels, num_overlapping_voxels, num_non_overlapping_voxels;
} vgx_voxel_evaluation_details;
VGX_API int vgx_evaluate_layers_rmse(vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode,
                                     vgx_voxel_evaluation_details* details,
                                     int32_t* error_block_index /* [n_test][3] or NULL */,
                                     float* error_distance /* [n_test][vps^3] or NULL */,
                                     uint8_t* error_set /* [n_test][vps^3] or NULL */, int32_t* n_error_blocks);

/* ---- Map queries: voxblox EsdfMap / TsdfMap lookups ----------------------- */
/* What a consumer of voxgraph's map asks of it: VoxgraphSubmap is a cblox::TsdfEsdfSubmap, and getEsdfMap() /
 * getTsdfMap() expose voxblox's EsdfMap / TsdfMap [recalled]: getDistanceAtPosition, getDistanceAndGradientAtPosition,
 * isObserved, getWeightAtPosition and their batchGet... forms, over Interpolator::getDistance / getGradient.  This call
 * answers n such questions about one finished submap's raw ESDF or TSDF layer (layer = VGX_EVAL_LAYER_ESDF / _TSDF).
 * The projected map becomes queryable through vgx_tsdf_layer_merge_submaps, vgx_submap_from_tsdf_layer and
 * vgx_submap_generate_esdf.  Everything about voxblox here is [recalled]: voxblox is not vendored.
 * Rules (what the kernel, vgx_query_kernel.h, and tests/map_query_ref.py all follow; f32, no contraction):
 *   point        without a pose p = the query point x.  With T_Q_S {qw,qx,qy,qz, tx,ty,tz}, p = T_S_Q * x, T_S_Q =
 *                T_Q_S.inverse() formed once in f32 as vgx_tsdf_layer_merge_submaps forms it (conjugate quaternion,
 *                translation -(q^-1 t)), applied as its transform_point (Eigen _transformVector, then + t).
 *   validity     an ESDF voxel is valid when observed != 0, a TSDF voxel when weight > 0.  A missing block is invalid.
 *   nearest      (getNearestDistance; flags without VGX_QUERY_INTERPOLATE) block b = floorf(p * block_size_inv + 1e-6f)
 *                per axis must exist; the voxel v = floorf((p - b * block_size) * voxel_size_inv + 1e-6f), clamped to
 *                [0, vps), must be valid; distance and (TSDF) weight are the voxel's own.
 *   interpolated (getInterpDistance; VGX_QUERY_INTERPOLATE) the 8 neighbours and the trilinear association of the
 *                isosurface points and the projected map (Interpolator::getVoxel(p, &v, true)); all 8 must exist and be
 *                valid.  A TSDF weight is interpolated the same way from the 8 weights.
 *   gradient     (getGradient; VGX_QUERY_GRADIENT) for each axis a in x, y, z and each sign s in -1, +1: d = the distance
 *                at p + s voxel_size e_a (the coordinate a alone changes: p_a - voxel_size, p_a + voxel_size), with the
 *                same interpolate flag; g_a = (d(+1) - d(-1)) / (2 voxel_size) (the sum s d, bit for bit).  Any of the six
 *                failing fails the query; p's own block must exist (implied: a valid distance at p reads it).  With a
 *                pose the gradient is rotated back into the query frame by q of T_Q_S (the rotation alone, not
 *                renormalised).  `valid` is then the conjunction of the gradient and the distance at p, as
 *                getDistanceAndGradientAtPosition returns it.
 *   invalid      an invalid query writes valid = 0 and +0.0f into every output it has (distance, gradient when asked
 *                for, weight when given); voxblox leaves the caller's values alone there (the C++ layer,
 *                voxgraph_amd/cpp/gpu_esdf_map.h, restores that).  A point with a coordinate |p_a * block_size_inv| >=
 *                2^30 -- every non-finite coordinate among them -- is invalid: the defined answer where voxblox's int
 *                cast of the block index is undefined.
 *   outputs      distance [n], gradient [n][3] (VGX_QUERY_GRADIENT only; not written otherwise), weight [n] (TSDF only;
 *                nullable), valid [n] u8 (1 / 0).
 * Refused with VGX_ERR_INVALID before anything is written (vgx_last_error says which): a NULL submap; n < 0; NULL points
 * / distance / valid with n > 0; VGX_QUERY_GRADIENT without a gradient array; a weight array on an ESDF query; unknown
 * flag bits or a layer value out of range; a layer the submap no longer holds in raw form (vgx_submap_release_raw_layers,
 * or an ESDF never generated); a pose that is not finite or whose |q.q - 1| > 1e-4.  n = 0: VGX_OK.
 * Streams and lifetimes: both calls run on the context's registration stream under the registration lock, ordered behind
 * vgx_submap_generate_esdf.  vgx_submap_query takes host arrays and returns with the results on the host;
 * vgx_submap_query_device takes device arrays and returns once the work is queued (vgx_ctx_synchronize waits for it).
 * One launch whatever n; values do not depend on scheduling. */
#define VGX_QUERY_INTERPOLATE 1 /* Interpolator::getDistance(.., interpolate = true); else the nearest voxel */
#define VGX_QUERY_GRADIENT 2    /* also Interpolator::getGradient (central differences, above)            */
VGX_API int vgx_submap_query(vgx_submap submap, int32_t layer, int32_t flags, const float T_Q_S[7] /* nullable */,
                             int64_t n, const float* points /* [n][3] */, float* distance /* [n] */,
                             float* gradient /* [n][3] or NULL */, float* weight /* [n] or NULL; TSDF only */,
                             uint8_t* valid /* [n] */);
VGX_API int vgx_submap_query_device(vgx_submap submap, int32_t layer, int32_t flags, const float T_Q_S[7] /* nullable, host */,
                                    int64_t n, const float* points, float* distance, float* gradient, float* weight,
                                    uint8_t* valid);

/* ---- Layer point clouds: voxblox_ros ptcloud_vis.h -------------------------- */
/* The point-cloud views of a layer that MapEvaluation publishes (map_evaluation.cpp:39, :105, :106):
 * createSurfaceDistancePointcloudFromTsdfLayer(gt TSDF, 0.6), createDistancePointcloudFromEsdfLayer(error layer) and
 * createDistancePointcloudFromEsdfLayerSlice(error layer, 2, 3 * voxel_size) -- and the same views of an active submap,
 * the projected map or a finished submap's ESDF.  A vgx_cloud holds the result on the device: per point the voxel centre
 * xyz [n][3] f32, intensity [n] f32 and, for VGX_CLOUD_SURFACE_COLOR, rgba [n][4] u8.  Everything about voxblox_ros here
 * is [recalled]: it is not vendored.
 * Rules (what the kernels, vgx_cloud.hip, and tests/layer_cloud_ref.py both follow; f32, no contraction):
 *   observed   an ESDF voxel when observed != 0; a TSDF voxel when weight > min_weight (strictly; a NaN weight is not
 *              observed).  min_weight defaults to ptcloud_vis.h's kMinWeight = 1e-3f [recalled] and is not used for ESDF
 *              sources.  The error layer of vgx_evaluate_layers_rmse_cloud is an ESDF-style layer: observed =
 *              error_set != 0, distance = e.
 *   kind       VGX_CLOUD_DISTANCE: every observed voxel (a distance that is NaN or infinite passes).
 *              VGX_CLOUD_SURFACE_DISTANCE: observed and fabsf(distance) < surface_distance (strictly; NaN and infinite
 *              distances fail).  VGX_CLOUD_SURFACE_COLOR: the same predicate, and the voxel's colour is copied, byte for
 *              byte, into rgba; only a vgx_tsdf_layer carries colours.
 *   slice      slice_axis -1: none.  Else a voxel also has to satisfy fabsf(c - slice_value) <= 0.5f * voxel_size + 1e-6f
 *              (not strictly), c its centre's coordinate on that axis: voxblox_ros' rule with voxblox's
 *              kFloatingPointTolerance = 1e-6 [recalled], here with the right-hand side formed in f32.  A plane on a
 *              block face (exactly half a voxel from the rows of centres on either side) therefore takes both rows,
 *              where those centres and the plane are exact in f32.  A block none of whose vps rows on that axis
 *              satisfies this is skipped without reading a voxel; the rows are tested with the very comparison above, so
 *              skipping never changes the result.
 *   position   the voxel centre origin + (idx + 0.5f) * voxel_size per axis, origin = (float)block_index * block_size,
 *              block_size = (float)vps * voxel_size -- exactly the centre of vgx_submap_extract_voxel_points and
 *              vgx_tsdf_layer_merge_submaps (one helper, vgx_internal.h voxel_centre), in the layer's own frame.
 *   intensity  the voxel's distance, bit for bit, for every kind.
 *   order      blocks in slot order -- the order of vgx_submap_block_index / vgx_tsdf_layer_download, and for
 *              vgx_evaluate_layers_rmse_cloud the error blocks' order (test-slot order) -- and inside a block the voxels
 *              in linear-index order (x fastest).  DEVIATION: voxblox walks its block hash map, whose order is not
 *              defined; this one is fixed, so a cloud is bit-identical run to run.
 * The handle is reused from call to call: its device buffers grow on demand; one call at a time per handle.
 * Refused with VGX_ERR_INVALID before anything is written, the cloud keeping what it held (vgx_last_error says which): a
 * NULL source or cloud, a cloud of another context, an unknown kind, a slice_axis outside [-1, 2], a surface_distance or
 * slice_value that is not finite, a min_weight that is negative or not finite (every field is checked whatever the kind),
 * VGX_CLOUD_SURFACE_COLOR on a submap layer or an error layer, a layer value that is neither VGX_EVAL_LAYER_ESDF nor
 * _TSDF, a submap layer that is no longer resident in raw form (vgx_submap_release_raw_layers, or an ESDF never
 * generated), and for vgx_evaluate_layers_rmse_cloud everything vgx_evaluate_layers_rmse refuses.  cfg == NULL: the
 * defaults.  VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16.  An empty result (an empty layer, nothing passes) is
 * VGX_OK with n_points = 0.  Out of device memory: VGX_ERR_NOMEM, and the cloud then holds 0 points.
 * Passes: count per block, rocprim exclusive scan, emit -- two kernels, one scan and one 8-byte memset whatever the size,
 * and two host synchronisations (the total, to size the output; the end).  Positions come from ballots and popcounts,
 * never from atomics.  vgx_submap_layer_cloud and vgx_evaluate_layers_rmse_cloud run on the registration stream under
 * the registration lock; vgx_tsdf_layer_cloud on the TSDF stream under the TSDF lock, behind the scans and merges already
 * queued (it launches one workgroup per slot of the layer's block pool and reads the allocation counter on the device, so
 * it does not wait for them first).  All three return with the cloud complete.
 * vgx_evaluate_layers_rmse_cloud is vgx_evaluate_layers_rmse and the cloud of its error layer in one call: it queues the
 * same kernels, keeps the error layer in device scratch that dies with the call, and brings back the details with the
 * point total -- nothing proportional to the layer crosses to the host.  *details is bit for bit what
 * vgx_evaluate_layers_rmse returns for the same arguments. */
#define VGX_CLOUD_DISTANCE 0
#define VGX_CLOUD_SURFACE_DISTANCE 1
#define VGX_CLOUD_SURFACE_COLOR 2
/* Fill it with vgx_cloud_config_default() before setting fields; every field is validated. */
typedef struct vgx_cloud_config {
  int32_t kind;           /* VGX_CLOUD_DISTANCE */
  float surface_distance; /* 0.6 (metres; what voxgraph passes, map_evaluation.cpp:39) */
  float min_weight;       /* 1e-3 (ptcloud_vis.h kMinWeight [recalled]) */
  int32_t slice_axis;     /* -1: no slice; 0, 1, 2: x, y, z */
  float slice_value;      /* 0: the plane's coordinate on slice_axis (metres) */
} vgx_cloud_config;
typedef struct vgx_cloud_s* vgx_cloud;
VGX_API void vgx_cloud_config_default(vgx_cloud_config* cfg);
VGX_API int vgx_cloud_create(vgx_ctx ctx, vgx_cloud* out);
VGX_API int vgx_cloud_destroy(vgx_cloud cloud);
/* any pointer may be NULL; *has_colors = 1 after a VGX_CLOUD_SURFACE_COLOR call */
VGX_API int vgx_cloud_stats(vgx_cloud cloud, int64_t* n_points, int32_t* has_colors);
/* xyz [n][3] f32, intensity [n] f32, rgba [n][4] u8; any may be NULL.  rgba on a cloud without colours: VGX_ERR_INVALID. */
VGX_API int vgx_cloud_download(vgx_cloud cloud, float* xyz, float* intensity, uint8_t* rgba);
/* DEVICE pointers to the same three arrays, for a consumer that stays on the device (NULL where the cloud has none: 0
 * points, no colours); valid until the next producing call on the handle or its destruction.  Any may be NULL. */
VGX_API int vgx_cloud_device_pointers(vgx_cloud cloud, const float** xyz, const float** intensity, const uint8_t** rgba);
/* a finished submap's raw layer: layer = VGX_EVAL_LAYER_ESDF / VGX_EVAL_LAYER_TSDF */
VGX_API int vgx_submap_layer_cloud(vgx_submap submap, int32_t layer, const vgx_cloud_config* cfg, vgx_cloud cloud);
/* a vgx_tsdf_layer: the active submap or the projected map, colours included */
VGX_API int vgx_tsdf_layer_cloud(vgx_tsdf_layer layer, const vgx_cloud_config* cfg, vgx_cloud cloud);
VGX_API int vgx_evaluate_layers_rmse_cloud(vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode,
                                           vgx_voxel_evaluation_details* details, const vgx_cloud_config* cfg,
                                           vgx_cloud cloud);

/* ---- Map messages: layers and the surface cloud as voxgraph publishes them ------ */
/* What voxgraph sends at the end of every submap and every optimisation: SubmapServer::publishSubmapTsdf /
 * publishSubmapTsdfAndEsdf (submap_server.cpp:83-105, cblox serializeSubmapToMsg), ProjectedMapServer::publishProjectedMap
 * (projected_map_server.cpp:21-38: voxblox::serializeLayerAsMsg<TsdfVoxel>(layer, false, &msg.tsdf_layer), action kReset)
 * and SubmapServer::publishSubmapSurfacePointcloud (submap_server.cpp:107-163: a PointCloud2 of pcl::PointXYZI) -- and
 * the receiving end, voxblox::deserializeMsgToLayer.  A vgx_map_msg holds one result on the device: a layer message
 * (block indices [n][3] i32 and words [n][vps^3 * W] u32) or a surface cloud (32 n bytes).  voxblox, cblox and PCL are
 * not vendored: the word formats, the three actions, the merge and the PointXYZI layout are [recalled].
 * Rules (what the kernels, vgx_msg.hip, and tests/map_msg_ref.py both follow; f32, no contraction):
 *   words       Block<TsdfVoxel>::serializeToIntegers: W = 3 words per voxel -- distance bits, weight bits,
 *               a | b << 8 | g << 16 | r << 24.  Block<EsdfVoxel>: W = 2 -- distance bits, observed ? 1 : 0 (parent bytes
 *               zero: this library keeps no parents).  Exactly what vgx_map_file_write emits for the same arrays
 *               (csrc/vgx_mapfile_schema.h).  Floats travel as bit patterns: NaN payloads and -0.0 survive.
 *   sources     a vgx_tsdf_layer (active submap, projected map: colours included); a finished submap's raw TSDF layer
 *               (its colour words when the submap has colours; a submap without colours writes colour word 0) or raw
 *               ESDF layer (layer = VGX_EVAL_LAYER_TSDF / _ESDF).
 *   order       blocks in slot order -- the order of vgx_tsdf_layer_download / vgx_submap_block_index -- voxels in
 *               linear-index order (x fastest).  only_updated = true (Update::kMap flags) does not exist here: nothing
 *               tracks updated blocks, and voxgraph passes false.
 *   actions     vgx_tsdf_layer_deserialize[_msg], MapDerializationAction's values [recalled].  VGX_MSG_ACTION_UPDATE: each
 *               message block replaces the layer's block of that index, allocated if absent (voxels and colours; colour
 *               bytes r g b a from the word above); other blocks are untouched.  VGX_MSG_ACTION_MERGE: an absent block
 *               is allocated and takes the message voxels; a present one gets mergeVoxelAIntoVoxelB(A = message voxel,
 *               B = layer voxel) per voxel: w' = wA + wB; if w' > 0, d = (dA*wA + dB*wB) / w', w = w' and the colour
 *               becomes Color::blendTwoColors as the integrators form it (per channel (uint8) roundf(cB * (wB / t) +
 *               cA * (wA / t)), t = wB + wA); else the voxel is unchanged (a NaN w' leaves it unchanged).  No weight
 *               cap.  VGX_MSG_ACTION_RESET: the layer is emptied, then UPDATE.
 *   surface     vgx_submap_surface_msg: point i of the device point set (the order of vgx_submap_download_points) fills
 *               bytes 32 i .. 32 i + 31: x y z FLOAT32 at 0 / 4 / 8, 1.0f at 12 (PCL's data[3]), intensity FLOAT32 at 16
 *               = the point's weight bit for bit, bytes 20..31 zero -- pcl::PointXYZI as pcl::toROSMsg lays it out:
 *               point_step 32, height 1, width n, row_step 32 n, little-endian, is_dense 1.  T == NULL copies the
 *               positions bit for bit; else T is a row-major 3 x 4 f32 affine applied as pcl::transformPoint does: per
 *               row ((m0*x + m1*y) + m2*z) + t.  Making T from a pose (T_B_S) is the caller's business
 *               (voxgraph_amd/cpp/gpu_map_messages.h does it).  vgx_scan_decode_msg_device reads these bytes back with
 *               the layout {point_step 32, offsets 0 / 4 / 8, VGX_SCAN_COLOR_INTENSITY at 16}.
 * The handle is reused from call to call: its device buffers grow on demand; one call at a time per handle.
 * Refused with VGX_ERR_INVALID before anything is written (vgx_last_error says which) -- by the producers, the handle
 * keeping what it held: a NULL source or message, a message of another context, a layer value that is neither
 * VGX_EVAL_LAYER_ESDF nor _TSDF, a submap layer no longer resident in raw form (vgx_submap_release_raw_layers, or an ESDF
 * never generated), an unknown point type, a point set that was never extracted or uploaded, a T entry that is not finite;
 * by the deserialising calls, the layer unchanged: a voxels_per_side other than the layer's, a voxel_size further than
 * 1e-5 from the layer's (deserializeMsgToLayer's kVoxelSizeEpsilon [recalled]), a layer type that is not TSDF (an ESDF
 * message handle included), a words length other than n_blocks * vps^3 * 3, an unknown action, n_blocks < 0, NULL arrays
 * with n_blocks > 0, a handle that holds no layer message, and the same block index twice (DEVIATION: voxblox would apply
 * duplicates in order).  n_blocks = 0: VGX_OK; with VGX_MSG_ACTION_RESET it empties the layer.  Deserialising an ESDF
 * message into a submap does not exist: submaps are immutable, a caller decodes on the host and uses vgx_submap_create.
 * VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16.  Out of device memory: VGX_ERR_NOMEM; a producer's handle then
 * holds nothing, a deserialising call has reserved the table and the pool for every message block before it touches a
 * voxel and leaves the layer unchanged.
 * Streams and locks: vgx_tsdf_layer_serialize and both deserialising calls run on the TSDF stream under the TSDF lock,
 * behind the scans and merges already queued; vgx_submap_serialize_layer and vgx_submap_surface_msg on the registration
 * stream under the registration lock.  A layer serialisation is one kernel and one device-to-device copy of the block
 * indices whatever the size, with at most two host synchronisations (the block total of a vgx_tsdf_layer, which only the
 * device knows -- the kernel still reads the allocation counter there and never passes it; the end); the surface cloud is
 * one kernel and one synchronisation.  A deserialisation is at most four memsets (RESET) and one kernel; values never
 * depend on scheduling, the slots of newly allocated blocks may, as after a scan.  Every call returns with its result
 * complete; the host-array form has read the caller's arrays by then. */
#define VGX_MSG_NONE 0 /* a new handle, or one whose last producer failed */
#define VGX_MSG_TSDF_LAYER 1
#define VGX_MSG_ESDF_LAYER 2
#define VGX_MSG_SURFACE_CLOUD 3
#define VGX_MSG_ACTION_UPDATE 0 /* voxblox MapDerializationAction::kUpdate [recalled] */
#define VGX_MSG_ACTION_MERGE 1
#define VGX_MSG_ACTION_RESET 2
typedef struct vgx_map_msg_s* vgx_map_msg;
VGX_API int vgx_map_msg_create(vgx_ctx ctx, vgx_map_msg* out);
VGX_API int vgx_map_msg_destroy(vgx_map_msg msg);
/* any pointer may be NULL.  *n: blocks, or points; *words_per_voxel: 3, 2, or 0 for a cloud; *n_bytes: of the payload
 * (words, or cloud data) */
VGX_API int vgx_map_msg_stats(vgx_map_msg msg, int32_t* kind, int64_t* n, int32_t* words_per_voxel, int64_t* n_bytes);
/* the voxel size and voxels per side of the layer a layer message was made from (VGX_ERR_INVALID otherwise) */
VGX_API int vgx_map_msg_layer_geometry(vgx_map_msg msg, float* voxel_size, int32_t* voxels_per_side);
/* block_index [n][3] i32 (layer messages only), payload n_bytes bytes; either may be NULL */
VGX_API int vgx_map_msg_download(vgx_map_msg msg, int32_t* block_index, void* payload);
/* DEVICE pointers to the same two arrays (NULL where the message has none); valid until the next producing call on the
 * handle or its destruction.  Either may be NULL. */
VGX_API int vgx_map_msg_device_pointers(vgx_map_msg msg, const int32_t** block_index, const void** payload);
/* voxblox::serializeLayerAsMsg(layer, only_updated = false) of a vgx_tsdf_layer: the active submap, the projected map */
VGX_API int vgx_tsdf_layer_serialize(vgx_tsdf_layer layer, vgx_map_msg msg);
/* ... of a finished submap's raw layer: layer = VGX_EVAL_LAYER_TSDF / VGX_EVAL_LAYER_ESDF */
VGX_API int vgx_submap_serialize_layer(vgx_submap submap, int32_t layer, vgx_map_msg msg);
/* the data bytes of publishSubmapSurfacePointcloud's PointCloud2; point_type = VGX_POINTS_ISOSURFACE / _VOXELS */
VGX_API int vgx_submap_surface_msg(vgx_submap submap, int32_t point_type, const float* T /* [12] row-major 3 x 4, or NULL */,
                                   vgx_map_msg msg);
/* voxblox::deserializeMsgToLayer from host arrays: layer_type = VGX_EVAL_LAYER_TSDF (anything else is refused),
 * block_index [n_blocks][3], words [n_words], n_words = n_blocks * vps^3 * 3 */
VGX_API int vgx_tsdf_layer_deserialize(vgx_tsdf_layer layer, int32_t action, int32_t layer_type, double voxel_size,
                                       int32_t voxels_per_side, int32_t n_blocks, const int32_t* block_index,
                                       const uint32_t* words, int64_t n_words);
/* ... from a handle that holds a TSDF layer message: no host copy of the words */
VGX_API int vgx_tsdf_layer_deserialize_msg(vgx_tsdf_layer layer, int32_t action, vgx_map_msg msg);

/* ---------------------------------------------------------------------------
 * Saved maps: cblox submap-collection files and voxblox layer files.
 *
 * voxgraph saves its map with SubmapCollection::saveToFile (voxgraph_mapper.cpp:412-417)
 * and reads collections back with cblox::io::LoadSubmapCollection<VoxgraphSubmap>
 * (registration_test_bench.cpp:173-175 -> VoxgraphSubmap::LoadFromStream,
 * voxgraph_submap.cpp:398-415).  The container is a sequence of length-prefixed
 * protobuf messages (varint32 size, then the message):
 *   collection : SubmapCollectionProto, then per submap a SubmapProto header followed by
 *                its TSDF BlockProtos and (TsdfEsdfSubmap) its ESDF BlockProtos
 *   layer file : varint32 message count, LayerProto, BlockProtos   (voxblox::io::SaveLayer)
 * This is a hand-written wire-format reader/writer (protobuf is not a dependency).
 * [recalled] The message schemas live in un-vendored voxblox / cblox and could not be
 * checked against a real file in this environment; they are isolated in one table
 * (voxgraph_amd/csrc/vgx_mapfile_schema.h).  Unknown fields are skipped, packed and
 * unpacked repeated encodings are both accepted.
 * Host-only (no device needed) except vgx_map_file_load_submap.
 * ------------------------------------------------------------------------- */
typedef struct vgx_map_file_s* vgx_map_file;
#define VGX_FILE_CBLOX_COLLECTION 0
#define VGX_FILE_VOXBLOX_LAYER 1
typedef struct vgx_map_file_submap_info {
  int64_t id;              /* SubmapProto.id (0 for a layer file)                       */
  double T_M_S[7];         /* submap pose {qw,qx,qy,qz, tx,ty,tz} (identity for a layer) */
  double voxel_size;
  int32_t voxels_per_side;
  int32_t n_tsdf_blocks;
  int32_t n_esdf_blocks;   /* 0 when the file holds no ESDF for this submap              */
  int32_t layer_is_esdf;   /* layer files only: LayerProto.type == "esdf"                */
} vgx_map_file_submap_info;
/* Indexes the file (headers and message offsets; voxel payloads are decoded on read). */
VGX_API int vgx_map_file_open(const char* path, int32_t format, vgx_map_file* out);
VGX_API int vgx_map_file_close(vgx_map_file file);
/* Last error of this file handle (or of the last failed open when file == NULL). */
VGX_API const char* vgx_map_file_last_error(vgx_map_file file);
VGX_API int32_t vgx_map_file_num_submaps(vgx_map_file file);
VGX_API int vgx_map_file_get_submap_info(vgx_map_file file, int32_t index, vgx_map_file_submap_info* info);
/* Decodes submap `index` into caller arrays (any may be NULL): TSDF blocks in file order
 * (block_index [n_tsdf][3], distance / weight / rgba [n_tsdf][vps^3]), and the ESDF values
 * of the SAME blocks (esdf_distance, esdf_observed [n_tsdf][vps^3]; blocks without an ESDF
 * counterpart read distance 0 / observed 0) -- the layout vgx_submap_create takes. */
VGX_API int vgx_map_file_read_submap(vgx_map_file file, int32_t index, int32_t* block_index,
                                     float* tsdf_distance, float* tsdf_weight, uint8_t* tsdf_rgba,
                                     float* esdf_distance, uint8_t* esdf_observed);
/* read + vgx_submap_create: the device-side counterpart of VoxgraphSubmap::LoadFromStream.
 * The submap is NOT finished: follow with vgx_submap_generate_esdf (if the file has no ESDF)
 * and the extract calls, as finishSubmap() does after loading. */
VGX_API int vgx_map_file_load_submap(vgx_ctx ctx, vgx_map_file file, int32_t index, vgx_submap* out);
/* Writer (round trips, and saving maps built on the device).  One entry per submap;
 * esdf_* may be NULL (TSDF-only submap). */
typedef struct vgx_map_file_submap_data {
  int64_t id;
  double T_M_S[7];
  int32_t n_blocks;
  const int32_t* block_index;     /* [n][3] */
  const float* tsdf_distance;     /* [n][vps^3] */
  const float* tsdf_weight;
  const uint8_t* tsdf_rgba;       /* [n][vps^3][4] or NULL */
  const float* esdf_distance;     /* or NULL */
  const uint8_t* esdf_observed;
} vgx_map_file_submap_data;
VGX_API int vgx_map_file_write(const char* path, int32_t format, double voxel_size,
                               int32_t voxels_per_side, int32_t n_submaps,
                               const vgx_map_file_submap_data* submaps);

/* ---- Pose graph: the solve ----------------------------------------------- */
/* PoseGraph::optimize() (voxgraph/src/backend/pose_graph.cpp:85-106) as a library call: Levenberg-Marquardt over the
 * 4-DoF poses {x, y, z, yaw} of the graph's nodes, the registration constraints evaluated by a vgx_reg_batch, the
 * relative-pose constraints (odometry, loop closures, heights: RelativePoseCostFunction,
 * relative_pose_cost_function_inl.h:8-70) on the host in f64, and the damped normal equations assembled, factorised
 * (Cholesky) and solved on the device in f64.  No robust loss (the reference passes none, constraint.h:34).  Two linear
 * solvers.  The default, VGX_LINEAR_SOLVER_DENSE, has no ordering and no sparsity: the reduced matrix is DENSE,
 * (4 x free nodes)^2 doubles twice over -- more than 4096 free nodes are refused with VGX_ERR_UNSUPPORTED (4 GiB at the
 * limit).  VGX_LINEAR_SOLVER_TILE_SPARSE stores and factorises the 64 x 64 tiles that are structurally non-zero alone
 * and has no such limit ("Pose graph: the tile-sparse solver" below).
 *
 * THE LOOP (what harness/lm.py restates for Ceres' trust-region minimiser).  Per iteration, at the accepted poses x
 * with cost, gradient g and Gauss-Newton matrix H over the free variables in ascending node order:
 *   stop GRADIENT_TOLERANCE when max |g| <= gradient_tolerance;
 *   D^2 = clip(diag(H), 1e-6, 1e32), A = H + diag(D^2 / radius), step = -A^-1 g (Cholesky; a pivot that is not
 *   positive or not finite: radius /= decrease, decrease *= 2, next iteration);
 *   stop PARAMETER_TOLERANCE when |step| <= parameter_tolerance * (|x_free| + parameter_tolerance);
 *   candidate = x + step, every yaw wrapped as a - 2 pi floor((a + pi) / 2 pi); its cost by a COST-ONLY evaluation
 *   (vgx_reg_batch_evaluate_cost); gain ratio rho = (cost - trial cost) / -(g.step + 0.5 step.(H step)), -1 when the
 *   model does not decrease;
 *   rho > 1e-3: accept -- one full evaluation at the candidate, radius = min(radius / max(1/3, 1 - (2 rho - 1)^3),
 *   1e16), decrease = 2, stop FUNCTION_TOLERANCE when |cost change| / cost <= function_tolerance;
 *   else radius /= decrease, decrease *= 2;
 *   stop MAX_SOLVER_TIME / MAX_ITERATIONS.
 * cost = 0.5 (registration + edges); the registration cost is the per-constraint costs added in list order from 0.0,
 * for both kinds of evaluation, so a trial cost and the full evaluation at the same poses agree bit for bit
 * (all-points batches; a sampling batch draws anew at every evaluation, and the full one's cost is then kept).
 *
 * THE ORDER CONTRACT.  Every number of a solve is reproducible from a sequential restatement
 * (tests/pose_graph_ref.py), bit for bit:
 *   assembly   every 4x4 block of H is 0.0 plus its contributions in this order: the fused buffer's diagonal block;
 *              the registration off-diagonal blocks in constraint-list order (constraint c = (a, b): off[c] at (a, b),
 *              its transpose at (b, a)); the edges in list order (aa, bb, ab, ab^T).  g likewise.  No atomics.
 *   Cholesky   right-looking, 64-wide panels; every element's history is a_ij <- a_ij - l_ik l_jk for k ascending,
 *              one rounded multiply and one rounded subtract at a time, then one division by l_jj (one sqrt on the
 *              diagonal): the blocked factor IS the unblocked right-looking one.  No FMA, no f64 MFMA.
 *   solves     column-oriented forward and back substitution, the same per-element order; H step: per row, ascending
 *              columns, from 0.0; the host's dot products and norms: ascending, from 0.0.
 *
 * vgx_pose_graph_create: n_nodes nodes; constant[i] != 0 fixes node i (the reference fixes the first submap,
 * pose_graph_interface.cpp:30-32, and every reference-frame node).  constant == NULL: node 0 alone is constant.
 * vgx_pose_graph_set_registration: the registration constraints, or NULL for none.  The batch is NOT owned; it must
 * hold the whole list (n_global == n) over node indices < n_nodes.  Destroying a batch a graph was given is deferred
 * until the graph lets go of it (another batch, NULL, or vgx_pose_graph_destroy); the graph refuses to solve meanwhile.
 * vgx_pose_graph_set_edges: replaces the list of relative-pose edges (allowed between solves): residual =
 * sqrt_information * [R(yaw_a)^T (t_b - t_a) - t_obs, normalize(yaw_b - yaw_a - yaw_obs)], sqrt_information a full
 * row-major 4x4 (the reference multiplies by a matrix, :60).  An absolute constraint is an edge from a constant
 * reference-frame node.  Refused with VGX_ERR_INVALID, the list left as it was: n_edges < 0 or NULL edges, an edge that
 * names a node out of range or joins a node to itself, an edge whose t_obs, yaw_obs or sqrt_information is not finite. */
typedef struct vgx_pose_graph_s* vgx_pose_graph;
typedef struct vgx_pose_graph_edge {
  int32_t a, b;
  double t_obs[3];
  double yaw_obs;
  double sqrt_information[16];
} vgx_pose_graph_edge;
typedef struct vgx_pose_graph_options {
  double parameter_tolerance;              /* 3e-3 (pose_graph.cpp:93) */
  double function_tolerance;               /* 1e-6  */
  double gradient_tolerance;               /* 1e-10 */
  double max_solver_time_in_seconds;       /* 4 (pose_graph.cpp:95) */
  double initial_trust_region_radius;      /* 1e4   */
  int32_t max_num_iterations;              /* 50    */
  int32_t exclude_registration_constraints; /* 0; pose_graph.cpp:74-83: the first stage after a loop closure */
} vgx_pose_graph_options;
/* ceres::TerminationType */
#define VGX_CONVERGENCE 0
#define VGX_NO_CONVERGENCE 1
#define VGX_FAILURE 2
/* which rule ended the solve */
#define VGX_TERMINATION_PARAMETER_TOLERANCE 0
#define VGX_TERMINATION_FUNCTION_TOLERANCE 1
#define VGX_TERMINATION_GRADIENT_TOLERANCE 2
#define VGX_TERMINATION_MAX_ITERATIONS 3
#define VGX_TERMINATION_MAX_SOLVER_TIME 4
#define VGX_TERMINATION_NO_FREE_NODES 5
typedef struct vgx_pose_graph_summary {
  int32_t termination_type;         /* VGX_CONVERGENCE / VGX_NO_CONVERGENCE / VGX_FAILURE */
  int32_t termination_reason;       /* VGX_TERMINATION_* */
  int32_t num_iterations;
  int32_t num_successful_steps;
  int32_t num_full_evaluations;     /* residuals and Jacobians: the first one and one per accepted step */
  int32_t num_cost_evaluations;     /* cost only: one per trial step */
  int32_t num_factorization_failures;
  int32_t num_free_nodes;
  double initial_cost, final_cost;
  double total_seconds;
  double registration_seconds;      /* inside the vgx_reg_batch evaluations (launch to result on the host) */
  double linear_algebra_seconds;    /* damping, factorisation, substitutions, H step (launch to result on the host) */
} vgx_pose_graph_summary;
/* one record per iteration of the last solve; what an iteration did not get to is 0 */
typedef struct vgx_pose_graph_iteration {
  double cost;          /* at the accepted poses the iteration started from */
  double trial_cost;
  double gain_ratio;
  double radius;        /* the radius the step was computed with */
  double step_norm;
  int32_t accepted;
  int32_t factorization_failed;
} vgx_pose_graph_iteration;
VGX_API int vgx_pose_graph_create(vgx_ctx ctx, int32_t n_nodes, const int32_t* constant /* [n_nodes] or NULL */,
                                  vgx_pose_graph* out);
VGX_API int vgx_pose_graph_destroy(vgx_pose_graph graph);
VGX_API int vgx_pose_graph_set_registration(vgx_pose_graph graph, vgx_reg_batch batch);
VGX_API int vgx_pose_graph_set_edges(vgx_pose_graph graph, int32_t n_edges, const vgx_pose_graph_edge* edges);
VGX_API void vgx_pose_graph_options_default(vgx_pose_graph_options* options);
/* poses: host [n_nodes][4] f64, in and out (constant nodes keep their position; every yaw comes back wrapped once a
 * step was tried).  options NULL: the defaults.  summary nullable.  Synchronous; one call at a time per graph.
 * Refused with VGX_ERR_INVALID (vgx_last_error says which): NULL graph or poses, a graph with neither registration
 * constraints nor edges, a batch that was destroyed, is sharded, or names a node >= n_nodes, a pose that is not finite.
 * A graph whose nodes are all constant returns VGX_OK at once with zero iterations. */
VGX_API int vgx_pose_graph_optimize(vgx_pose_graph graph, const vgx_pose_graph_options* options, double* poses,
                                    vgx_pose_graph_summary* summary);
/* the last solve's iterations: *n_iterations (nullable) = their number; the first min(capacity, n) are written */
VGX_API int vgx_pose_graph_history(vgx_pose_graph graph, int32_t capacity, vgx_pose_graph_iteration* iterations,
                                   int32_t* n_iterations);
/* the reduced normal equations at the poses the last solve ended at (its last full evaluation): n_free_variables
 * (nullable) = 4 x free nodes = N; H host [N][N] row-major and g host [N], either nullable. */
VGX_API int vgx_pose_graph_download_system(vgx_pose_graph graph, int32_t* n_free_variables, double* H, double* g);
/* The factorisation on its own, for a caller with a trust-region loop of their own: solves A x = b for a symmetric
 * positive definite A (host row-major [n][n], the LOWER triangle is read), b and x host [n]; L (nullable) host [n][n]
 * receives the Cholesky factor, zeros above the diagonal.  1 <= n <= 16384.  VGX_ERR_NOT_POSITIVE_DEFINITE when a
 * pivot is not positive or not finite (x and L are then unspecified); the solve above uses the same kernels. */
VGX_API int vgx_dense_spd_solve(vgx_ctx ctx, int32_t n, const double* A, const double* b, double* x, double* L);

/* ---- Pose graph: edge covariances ----------------------------------------- */
/* PoseGraph::getEdgeCovarianceMap (pose_graph.cpp:117-163) as a library call: ceres::Covariance::Compute over the whole
 * problem followed by GetCovarianceBlock per pair.  One full evaluation at `poses` (registration through the batch
 * unless excluded), H assembled by the lists of the solve, factorised UNDAMPED by the same Cholesky, and the columns of
 * H^-1 that the pairs name solved on the device: L L^T X = E, E the identity's columns of the distinct second nodes
 * (of pairs between two free nodes) in ascending free position, built on the device.
 *
 * covariance[p] (row-major 4x4) = rows of node pairs[2p], columns of node pairs[2p + 1] of H^-1: the solution columns
 * of node b = pairs[2p + 1] at the rows of node a = pairs[2p].  The computed inverse is not exactly symmetric, so
 * (a, b) and (b, a) are two answers, each defined on its own; (a, a) and duplicates are allowed.  A pair that names a
 * constant node gets sixteen zeros (as Ceres gives).
 *
 * THE ORDER CONTRACT, extended.  For every element of every solved column:
 *   forward    y_i = (b_i - l_i0 y_0 - l_i1 y_1 - ...) / l_ii, k ascending;
 *   backward   x_i = (y_i - l_ki x_k - ...) / l_ii, k descending from n - 1;
 * each term one rounded multiply and one rounded subtract -- tests/pose_graph_ref.py's forward / backward applied to the
 * column (tests/pose_graph_covariance_ref.py).  Rows above a unit column's 1 are not computed in the forward pass (they
 * are +0.0 for a factor that passed the pivot check) and rows above the lowest one wanted are not computed in the
 * backward pass: no delivered bit depends on either.
 *
 * poses host [n_nodes][4] f64, read only.  Synchronous, two host synchronisations (the evaluation's and the result's),
 * one device-to-host copy.  The solved columns are held by the graph, grown on demand: at most (4 x free nodes)^2
 * doubles, 2 GiB at the 4096-node limit.  Afterwards vgx_pose_graph_download_system returns the H, g of this evaluation.
 * VGX_ERR_NOT_POSITIVE_DEFINITE when a pivot is not positive or not finite -- a rank-deficient graph, e.g. a free node
 * that no constraint touches; `covariance` is then unspecified.  Refused with VGX_ERR_INVALID (vgx_last_error says
 * which): NULL graph; NULL poses, pairs or covariance while n_pairs > 0; n_pairs < 0; a node index out of range; a pose
 * that is not finite; the graph states vgx_pose_graph_optimize refuses.  A refused call leaves `covariance` untouched.
 * n_pairs == 0 is VGX_OK and does nothing; a graph whose nodes are all constant returns zeros.  More than 2^26 pairs in
 * one call: VGX_ERR_UNSUPPORTED. */
VGX_API int vgx_pose_graph_covariance(vgx_pose_graph graph, const double* poses /* [n_nodes][4] */,
                                      int32_t exclude_registration_constraints,
                                      int32_t n_pairs, const int32_t* pairs /* [n_pairs][2] */,
                                      double* covariance /* [n_pairs][16] */);
/* The same kernels on a caller's matrix and general right-hand sides: solves A X = B for a symmetric positive definite
 * A (host row-major [n][n], the LOWER triangle is read), B and X host [n][m] row-major (they may be the same array); L
 * (nullable) as for vgx_dense_spd_solve.  1 <= n <= 16384, 1 <= m <= 16384.  Column c of X is bit for bit what
 * vgx_dense_spd_solve returns for column c of B.  VGX_ERR_NOT_POSITIVE_DEFINITE as there (X and L then unspecified). */
VGX_API int vgx_dense_spd_solve_many(vgx_ctx ctx, int32_t n, const double* A, int32_t m,
                                     const double* B /* [n][m] */, double* X /* [n][m] */, double* L /* nullable */);

/* ---- Pose graph: the tile-sparse solver ------------------------------------ */
/* The reference hands its problem to SPARSE_SCHUR (pose_graph.cpp:97).  VGX_LINEAR_SOLVER_TILE_SPARSE is the same
 * right-looking 64-wide-panel Cholesky over a tile table: H and A / L are arrays of 64 x 64 f64 tiles (32 KiB each,
 * row-major inside a tile, 16 nodes per tile), and a tile that is structurally zero in L is never stored, read or updated.
 *
 * STRUCTURE (host, made with the assembly's lists: whenever the constraints changed or registration is switched off
 * or on).  The block graph has one vertex per free node and an edge per registration constraint and per relative-pose
 * edge between two free nodes.  Tile (I, J) of H is stored when some 4x4 block of it is touched -- a joined pair at
 * positions a, b with a / 16 == I, b / 16 == J -- and every diagonal tile is.  L's tiles are H's lower ones plus the
 * symbolic fill at tile granularity: K ascending, every I >= J > K with (I, K) and (J, K) stored adds (I, J).  Per
 * panel K: its stored tiles below the diagonal, and the update triples (target (I, J), sources (I, K), (J, K)).
 *
 * ORDERING decides the fill.  VGX_ORDER_NATURAL: the free nodes ascending.  VGX_ORDER_RCM: reverse Cuthill-McKee on
 * the block graph, deterministic -- components in ascending order of their lowest node, each started at its
 * minimum-degree node (ties: the lowest index), breadth-first, a node's new neighbours appended by ascending (degree,
 * index), the whole sequence reversed.  VGX_ORDER_GIVEN: the caller's permutation, permutation[p] = the free node (its
 * index among the free nodes) at position p.  With an order P other than natural the system solved is P H P^T: g goes
 * in permuted, the step and H step come out in ascending node order, and the host's dot products and norms stay in
 * ascending node order.
 *
 * THE ORDER CONTRACT, extended.  Assembly: the same lists, sources and order, stored at (tile, in-tile) addresses.
 * Cholesky: every STORED element keeps the history a_ij <- a_ij - l_ik l_jk for k ascending, then one division or one
 * sqrt; the only terms left out are products with an exact zero factor (a tile not stored).  So the factor EQUALS the
 * dense solver's on P H P^T (tests/pose_graph_sparse_ref.py restates it bit for bit); it can differ in the sign of a
 * zero alone: the dense -0.0 - (-0.0) is +0.0 where the sparse solver leaves -0.0.  Substitutions: after a panel's
 * triangle only the rows (forward) / columns (backward) of the stored tiles are updated, the per-element k order
 * unchanged.  H step: per row of P H P^T, ascending columns over the row's stored tiles, from 0.0.  A fill tile starts
 * at +0.0.  A matrix with an inf or NaN off the diagonal is outside the equality (the dense solver multiplies it by
 * the zeros this one skips); the bad-pivot rule itself is unchanged.
 *
 * LAUNCHES.  Three per panel (diagonal tile; the column's stored tiles; the panel's triples), one for a panel with an
 * empty column below the diagonal; no workgroup waits for another, no cooperative launch, no captured graph.  A long
 * graph is launch-bound: supernodes and level scheduling of independent panels are not done.
 *
 * LIMITS.  The free-node limit (4096) applies to the dense solver alone.  THE TILE CAP: the tiles of H and L together
 * must fit the device memory that is free when the structure is made (hipMemGetInfo, less the graph's vectors), at
 * 32 KiB a tile; a structure over it is refused with VGX_ERR_UNSUPPORTED by the call that makes the lists
 * (vgx_pose_graph_optimize), the error text naming both figures.  The cap is taken at that moment: on a device that
 * other processes allocate from, a structure accepted once can be refused the next time the lists are made, and the
 * reverse.  At most 2^27 free nodes.  The host lists and the structure are sized by the graph: out of host memory is
 * VGX_ERR_NOMEM from the same calls (and from vgx_pose_graph_tile_pattern and vgx_block_spd_solve).
 * vgx_pose_graph_covariance keeps the DENSE factor and its limit whatever the solver setting: on a graph with more than
 * 4096 free nodes it returns VGX_ERR_UNSUPPORTED, `covariance` untouched; vgx_pose_graph_covariance_sparse ("Pose graph:
 * edge covariances on the tile-sparse factor" below) solves the same columns on the sparse factor and has no such limit.
 * vgx_pose_graph_download_system in sparse mode returns H dense, in ascending node order, when
 * 4 x free nodes <= 16384; beyond, VGX_ERR_UNSUPPORTED with g still delivered. */
#define VGX_LINEAR_SOLVER_DENSE 0
#define VGX_LINEAR_SOLVER_TILE_SPARSE 1
#define VGX_ORDER_NATURAL 0
#define VGX_ORDER_RCM 1
#define VGX_ORDER_GIVEN 2
typedef struct vgx_pose_graph_structure_stats {
  int32_t n_free_variables;   /* 4 x free nodes */
  int32_t n_panels;           /* tile rows */
  int32_t n_launches;         /* per factorisation */
  int32_t reserved;
  int64_t n_h_tiles;          /* stored tiles of H (both triangles) */
  int64_t n_l_tiles;          /* stored tiles of L: H's lower ones and the fill */
  int64_t n_update_triples;
  int64_t bytes;              /* device bytes of the tiles and the lists */
} vgx_pose_graph_structure_stats;
/* Allowed between solves.  permutation: [free nodes] for VGX_ORDER_GIVEN (copied), ignored otherwise; the dense solver
 * ignores the ordering.  VGX_ERR_INVALID: an unknown solver or ordering, a permutation that is NULL or not one;
 * VGX_ERR_UNSUPPORTED: the dense solver on a graph with more than 4096 free nodes.  A refused call changes nothing. */
VGX_API int vgx_pose_graph_set_linear_solver(vgx_pose_graph graph, int32_t solver, int32_t ordering,
                                             const int32_t* permutation /* [free nodes] or NULL */);
/* vgx_pose_graph_create with the solver chosen at creation.  vgx_pose_graph_create makes a DENSE graph and keeps
 * refusing more than 4096 free nodes; a graph past that limit is created here with VGX_LINEAR_SOLVER_TILE_SPARSE. */
VGX_API int vgx_pose_graph_create_with_solver(vgx_ctx ctx, int32_t n_nodes, const int32_t* constant /* or NULL */,
                                              int32_t solver, int32_t ordering, const int32_t* permutation,
                                              vgx_pose_graph* out);
/* the structure in use; valid once the tile-sparse solver has made its lists (a solve since the last change of the
 * constraints or the solver), VGX_ERR_INVALID before */
VGX_API int vgx_pose_graph_structure(vgx_pose_graph graph, vgx_pose_graph_structure_stats* stats);
/* the order in use, permutation_out [free nodes]: position -> free node.  The identity for the dense solver.
 * VGX_ORDER_RCM is made with the lists: VGX_ERR_INVALID before the first solve. */
VGX_API int vgx_pose_graph_order(vgx_pose_graph graph, int32_t* permutation_out);
/* The structure alone, on the host: no context, no HIP call.  pairs [n_pairs][2]: the joined free nodes (indices among
 * the free nodes).  permutation: for VGX_ORDER_GIVEN.  permutation_out (nullable) [n_free_nodes]: the order; tiles
 * (nullable when capacity == 0) [capacity][2]: the first `capacity` tiles of L as (row, column), sorted by (column,
 * row); *n_tiles (nullable): their number.  VGX_ERR_INVALID: n_free_nodes < 1, a pair out of range, an unknown
 * ordering, a permutation that is not one.  VGX_ERR_NOMEM: out of host memory. */
VGX_API int vgx_pose_graph_tile_pattern(int32_t n_free_nodes, int32_t n_pairs, const int32_t* pairs, int32_t ordering,
                                        const int32_t* permutation, int32_t* permutation_out, int32_t capacity,
                                        int32_t* tiles, int32_t* n_tiles);
/* The same kernels on a caller's matrix, vgx_dense_spd_solve's sibling: A symmetric positive definite of 4 x
 * n_block_rows unknowns, given as the 4x4 blocks (row-major values[k], at block row bi[k], block column bj[k]) of its
 * LOWER triangle (of a diagonal block the lower triangle is read); blocks not given are zero.  Natural order.  b and x
 * host [4 n_block_rows].  stats nullable (n_h_tiles: the tiles the blocks touch).  tile_index (nullable)
 * [n_l_tiles][2] = (row, column) of the factor's tiles, tile_values (nullable) [n_l_tiles][4096] their values, zeros
 * above the diagonal and past the matrix; size them with vgx_pose_graph_tile_pattern.  VGX_ERR_INVALID: a block out of
 * range, above the diagonal or given twice.  VGX_ERR_UNSUPPORTED: the tile cap.  VGX_ERR_NOT_POSITIVE_DEFINITE as for
 * vgx_dense_spd_solve. */
VGX_API int vgx_block_spd_solve(vgx_ctx ctx, int32_t n_block_rows, int32_t nnz, const int32_t* bi, const int32_t* bj,
                                const double* values /* [nnz][16] */, const double* b, double* x,
                                vgx_pose_graph_structure_stats* stats, int32_t* tile_index, double* tile_values);

/* ---- Pose graph: edge covariances on the tile-sparse factor ---------------- */
/* vgx_pose_graph_covariance on the factor of the tile-sparse solver: the same blocks of H^-1, with no free-node limit
 * and without the dense factor's work on structural zeros.  The graph's solver must be VGX_LINEAR_SOLVER_TILE_SPARSE
 * (otherwise VGX_ERR_INVALID, the text pointing to vgx_pose_graph_covariance).  The call makes the sparse lists itself
 * when they are not there -- before any solve (so VGX_ORDER_RCM works before a solve too), or after
 * vgx_pose_graph_covariance has left dense lists behind -- and the tile cap can refuse it as it refuses
 * vgx_pose_graph_optimize.
 *
 * THE SYSTEM.  P H P^T, P the order in use (natural, RCM or given): one full evaluation at `poses`, H's tiles copied
 * into A's, factorised UNDAMPED by the tiled Cholesky.  THE COLUMNS solved are those of the distinct second nodes of
 * the pairs between two free nodes, in ascending POSITION under P, four per node: column k of a node at position q is
 * the identity's column 4 q + k.  covariance[p] = the solved columns of node pairs[2p + 1] at rows
 * 4 pos(pairs[2p]) .. + 3 -- since (P H P^T)^-1 = P H^-1 P^T that is block (a, b) of H^-1, whatever the order.  A pair
 * with a constant node gives sixteen zeros; (a, a), both directions of a pair and duplicates are allowed.
 *
 * THE ORDER CONTRACT.  Every delivered element has the history of tests/pose_graph_sparse_ref.py's forward and
 * backward applied to its column:
 *   forward    y_i = (b_i - l_i0 y_0 - l_i1 y_1 - ...) / l_ii, k ascending;
 *   backward   x_i = (y_i - l_ki x_k - ...) / l_ii, k descending;
 * each term one rounded multiply and one rounded subtract; the only terms left out are the products with a tile that
 * is not stored.  So
 *   - column c equals, bit for bit, what vgx_block_spd_solve -- or the graph's own tiled substitution -- gives for that
 *     right-hand side alone;
 *   - under the natural order the delivered blocks equal vgx_pose_graph_covariance's AS NUMBERS (-0.0 == +0.0): the
 *     products left out are exact zeros of a finite factor, which change no value, only possibly the sign of a zero.
 * Two skips, vgx_pose_graph_covariance's restated for positions under P: the forward pass of a workgroup (32 columns)
 * starts at the panel of its first column's 1 -- above it b_i = 0 and every y_k so far is +0.0, and with a finite
 * factor 0.0 - l * 0.0 = +0.0 and +0.0 / l_ii = +0.0, which is what the column holds already; the backward pass stops
 * after the panel of the lowest row its columns' pairs want, and updates no tile left of that panel -- the rows above
 * take no part in the rows below.  No delivered bit depends on either.  No other panel or tile is skipped.
 *
 * SLABS.  The solved columns live in X [4 x free nodes][S], S the largest multiple of 32 with
 * 8 (4 x free nodes) S <= max_solve_bytes (0: the default, 1 GiB), 32 at the least whatever the budget and no more
 * than the columns there are.  The columns are solved S at a time; chunks of 32 columns are independent, so the slab
 * width changes no bit.  Per slab four launches (unit columns, forward, backward, gather of the slab's pairs into the
 * one [n_pairs][16] device array); no workgroup waits for another, no cooperative launch, no captured graph.  The graph
 * holds the slab buffer, grown on demand and never past max(max_solve_bytes, 32 columns).  Synchronous, two host
 * synchronisations (the evaluation's and the result's).
 *
 * Refusals, VGX_ERR_NOT_POSITIVE_DEFINITE, n_pairs == 0, an all-constant graph and the 2^26 pair cap: as for
 * vgx_pose_graph_covariance; max_solve_bytes < 0: VGX_ERR_INVALID.  A refused call leaves `covariance` untouched.
 * Afterwards vgx_pose_graph_download_system returns this evaluation's H and g (the sparse-mode rules), and a later
 * vgx_pose_graph_optimize or vgx_pose_graph_covariance on the handle gives the bits it gives on a fresh handle. */
typedef struct vgx_pose_graph_covariance_stats {
  int32_t n_columns;   /* columns of H^-1 solved: 4 x distinct second nodes of pairs between free nodes */
  int32_t n_slabs;     /* column slabs the solve was cut into */
  int32_t n_launches;  /* after the evaluation: the copy of H's tiles + the factorisation's + 4 per slab (unit columns,
                        * forward, backward, gather) */
  int32_t reserved;
  int64_t solve_bytes; /* device bytes of the solved-column buffer actually used */
} vgx_pose_graph_covariance_stats;
VGX_API int vgx_pose_graph_covariance_sparse(vgx_pose_graph graph, const double* poses /* [n_nodes][4] */,
                                             int32_t exclude_registration_constraints,
                                             int32_t n_pairs, const int32_t* pairs /* [n_pairs][2] */,
                                             int64_t max_solve_bytes /* 0: the default, 1 GiB */,
                                             double* covariance /* [n_pairs][16] */,
                                             vgx_pose_graph_covariance_stats* stats /* nullable */);
/* The same kernels on a caller's matrix: vgx_block_spd_solve with m right-hand sides.  B and X host
 * [4 n_block_rows][m] row-major (they may be the same array), 1 <= m <= 16384.  Column c of X is bit for bit what
 * vgx_block_spd_solve returns for column c of B.  Refusals and VGX_ERR_NOT_POSITIVE_DEFINITE as there (X is then
 * unspecified). */
VGX_API int vgx_block_spd_solve_many(vgx_ctx ctx, int32_t n_block_rows, int32_t nnz, const int32_t* bi, const int32_t* bj,
                                     const double* values /* [nnz][16] */, int32_t m,
                                     const double* B /* [4 n_block_rows][m] */, double* X /* may be B */);

/* ---- Scan-to-map registration ---------------------------------------------- */
/* The refinement voxgraph_mapper.h:164 announces ("Map tracker handles the odometry input and refines it using
 * scan-to-map ICP") and the reference's MapTracker does not perform: a scan's sensor pose T_S_C refined against the
 * ACTIVE TSDF layer before the scan is integrated.  DEFINED HERE, not recalled: point-to-implicit-surface Gauss-Newton
 * over a 4-DoF correction, the formulation the registration cost function uses between submaps.  voxblox's own
 * mini-batch ICP class is a different scheme and is not restated.
 *
 * THE FORMULATION.  n sensor-frame points p_C (f32), a prior T_S_C = {qw,qx,qy,qz, tx,ty,tz} (f32, the integrator's
 * convention), a correction delta = (x, y, z, yaw) in f64 applied about the sensor's prior position in the layer frame.
 * All of the following in f32, one rounding per operation, no contraction:
 *   q   = R_prior p_C                         Eigen _transformVector (v + w uv + u x uv, uv = 2 u x v)
 *   c, s = (float)cos(yaw), (float)sin(yaw)   computed on the host in f64;  t' = (float)((double)t_prior + delta_xyz)
 *   p_S = ((c qx - s qy) + tx', (s qx + c qy) + ty', qz + tz')
 *   r   = D(p_S), the trilinear TSDF distance over the 8 neighbours (Interpolator<TsdfVoxel>: every neighbour's block
 *         exists and every weight is > 0, else the point is not usable)
 *   g_a = (dD/d dl_a) * voxel_size_inv, the exact derivative of the interpolant from the same 8 voxels:
 *         d/d dl0 = ((c1 + dl1 c4) + dl2 c6) + (dl1 dl2) c7, d/d dl1 = ((c2 + dl0 c4) + dl2 c5) + (dl2 dl0) c7,
 *         d/d dl2 = ((c3 + dl1 c5) + dl0 c6) + (dl0 dl1) c7 in the interpolant's coefficients
 *   J   = (g_x, g_y, g_z, g_x ((-s) qx - c qy) + g_y (c qx - s qy))
 * A point is a CANDIDATE when its index is a multiple of point_stride and |p_C|^2 = (x x + y y) + z z lies in
 * [min_range_m^2, max_range_m^2] (f32; a NaN fails).  A candidate is USABLE when |p_S_a * block_size_inv| < 2^30 on
 * every axis (so every non-finite point is skipped), the interpolation is valid and |D| < max_abs_distance_m (the
 * clamped free-space plateau has no gradient and says nothing about the pose).  SPECIAL VOXEL VALUES fall under these
 * comparisons as IEEE decides them: a weight that is NaN, -0.0, +0.0 or negative is not > 0 (the voxel is unobserved), a
 * denormal or +inf weight is; a NaN or infinite D -- any NaN or +-inf among the 8 distances -- fails |D| <
 * max_abs_distance_m and the point has no term; -0.0 and denormal distances are ordinary values (nothing is flushed).
 *
 * THE ORDER CONTRACT.  Per usable point 15 f64 terms: r r; J_k r (k = 0..3); J_k J_l for k <= l in the order 00 01 02
 * 03 11 12 13 22 23 33 -- products of two f32 values widened to f64, exact.  Only the additions round:
 *   candidate j (point j * point_stride) belongs to workgroup j / 1024, thread (j % 1024) % 256, trip (j % 1024) / 256;
 *   a thread adds its usable points' terms to 0.0 in ascending trip; the 64 lanes of a wave fold by
 *   v[l] += v[l + o], o = 32, 16, 8, 4, 2, 1; lane 0 of wave 0, then waves 1, 2, 3 added in order: one partial per
 *   workgroup.  The fold: partial b to thread b % 256 of ONE workgroup, added to 0.0 in ascending b; the same wave
 *   fold; the 4 waves in order.  The two counts (usable, candidates) are int64 sums.
 * The partition depends on n and point_stride alone, never on the device.  No float atomics; two launches and one host
 * synchronisation per evaluation (tests/scan_registration_ref.py restates every bit).  cost = 0.5 sum r r.
 *
 * THE LOOP is vgx_pose_graph_optimize's ("Pose graph: the solve") with one free node, x = delta starting at 0: the
 * same damping D^2 = clip(diag H, 1e-6, 1e32), A = H + diag(D^2 / radius), a 4x4 right-looking Cholesky on the host in
 * the same per-element order (a failed pivot shrinks the radius), column-oriented substitutions, the yaw wrap, the
 * gain ratio, the radius update and the five stopping rules.  ONE difference: there is no cost-only form -- every trial
 * step is a full evaluation, an accepted step keeps its g and H, a rejected one discards them; evaluations = 1 + trial
 * steps.  options->exclude_registration_constraints is ignored.
 *
 * THE OUTCOME.  usable = 1 iff the solve ended in VGX_CONVERGENCE and n_valid / n_candidates >= min_valid_ratio at
 * both the first and the last accepted evaluation.  Then T_refined = {q_z(yaw) (x) q_prior, t_prior + delta_xyz}, formed
 * in f64 from the f32 prior and rounded to f32 once; otherwise T_refined is the prior's bits, `delta` still what the
 * solve ended at.  A scan that cannot be registered is an answer, not an error: VGX_OK with usable = 0.  Too few
 * usable points at the prior: at once, zero iterations, termination VGX_FAILURE / VGX_TERMINATION_TOO_FEW_POINTS.
 *
 * The kernels run on the context's TSDF stream under the lock the integrators take: an evaluation is ordered behind
 * every scan already queued on that layer, and the scan never leaves the device.  One call at a time per handle.
 *
 * Points: _set_points copies host points; _set_points_device and _set_scan BORROW (a device array ready with respect
 * to the TSDF stream / a vgx_scan as it stands at each evaluation) until the next set or the handle's destruction.
 * Refused with VGX_ERR_INVALID, nothing written (vgx_last_error says which): NULL arguments; no points set; a layer or
 * scan of another context; a prior that is not finite or whose quaternion has | |q|^2 - 1 | > 1e-4; a delta that is not
 * finite; point_stride < 1; max_abs_distance_m <= 0 or not finite; min_range_m > max_range_m or a NaN range; a
 * min_valid_ratio that is not finite.  VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16; more than
 * (2^31 - 1) * 1024 candidates (one launch). */
typedef struct vgx_scan_registration_s* vgx_scan_registration;
typedef struct vgx_scan_registration_config {
  float min_range_m;         /* 0 */
  float max_range_m;         /* +inf */
  float max_abs_distance_m;  /* NO default (0: refused): below the layer's truncation distance, e.g. 0.55 of 0.6 m */
  int32_t point_stride;      /* 1 */
  float min_valid_ratio;     /* 0.5 */
} vgx_scan_registration_config;
#define VGX_TERMINATION_TOO_FEW_POINTS 6
typedef struct vgx_scan_registration_summary {
  int32_t usable;
  int32_t termination_type;    /* VGX_CONVERGENCE / VGX_NO_CONVERGENCE / VGX_FAILURE */
  int32_t termination_reason;  /* VGX_TERMINATION_* */
  int32_t num_iterations;
  int32_t num_successful_steps;
  int32_t num_evaluations;     /* 1 + trial steps */
  int32_t num_factorization_failures;
  int32_t reserved;
  int64_t n_candidates;
  int64_t n_valid_first, n_valid_last; /* usable points at the prior / at the correction the solve ended at */
  double initial_cost, final_cost;
  double total_seconds;
  double evaluation_seconds;   /* launch to result on the host, all evaluations */
} vgx_scan_registration_summary;
VGX_API void vgx_scan_registration_config_default(vgx_scan_registration_config* cfg);
VGX_API int vgx_scan_registration_create(vgx_ctx ctx, const vgx_scan_registration_config* cfg, vgx_scan_registration* out);
VGX_API int vgx_scan_registration_destroy(vgx_scan_registration reg);
VGX_API int vgx_scan_registration_set_points(vgx_scan_registration reg, const float* points /* host [n][3] */, int64_t n);
VGX_API int vgx_scan_registration_set_points_device(vgx_scan_registration reg, const void* d_points /* f32 [n][3] */, int64_t n);
VGX_API int vgx_scan_registration_set_scan(vgx_scan_registration reg, vgx_scan scan);
/* the normal equations at a given correction: out[15] = {sum r r, sum J_k r [4], sum J_k J_l [10]} */
VGX_API int vgx_scan_registration_evaluate(vgx_scan_registration reg, vgx_tsdf_layer layer, const float T_S_C_prior[7],
                                           const double delta[4], double out[15], int64_t* n_valid, int64_t* n_candidates);
/* options NULL: vgx_pose_graph_options_default.  T_refined [7] and delta [4] are written on VGX_OK; summary nullable. */
VGX_API int vgx_scan_registration_refine(vgx_scan_registration reg, vgx_tsdf_layer layer, const float T_S_C_prior[7],
                                         const vgx_pose_graph_options* options, float T_refined[7], double delta[4],
                                         vgx_scan_registration_summary* summary);
/* the last refinement's iterations, as vgx_pose_graph_history */
VGX_API int vgx_scan_registration_history(vgx_scan_registration reg, int32_t capacity, vgx_pose_graph_iteration* iterations,
                                          int32_t* n_iterations);

/* ---- Scan localisation ------------------------------------------------------- */
/* Where is the sensor in the map that is already finished?  A scan's points against the ESDF (or TSDF) of POSED,
 * FINISHED submaps: one evaluation at a pose, many poses scored in one call, the best one refined.  It serves
 * re-localisation after the tracker is lost, the check of a proposed loop closure before it becomes a relative-pose
 * edge, and the start pose when mapping resumes in a loaded map (vgx_map_file_load_submap).  DEFINED HERE, not recalled:
 * the reference takes loop closures from outside and never verifies them.
 *
 * THE HANDLE is vgx_scan_registration: its points (host, device, vgx_scan), ranges, point_stride, max_abs_distance_m
 * and min_valid_ratio apply unchanged, and vgx_scan_registration_history serves _refine_map and _localize too.
 * vgx_scan_registration_set_map lists 1 <= n <= 64 finished submaps of the handle's context and of ONE voxels_per_side
 * (8 or 16; voxel sizes may differ), each with a general unit-quaternion pose T_M_S (M: the mission frame).  T_S_M is
 * formed once in f32 by vgx_submap_query's rule (conjugate rotation, translation -(q^-1 t)).  The handle takes a user
 * count on every listed submap, as vgx_reg_create does: a vgx_submap_destroy meanwhile is deferred to the next _set_map
 * or the handle's destruction.  n_submaps = 0 clears the map.  A submap whose chosen layer is no longer resident
 * (vgx_submap_release_raw_layers, or an ESDF never generated) is refused by the next evaluation, VGX_ERR_INVALID.
 *
 * THE FORMULATION.  f32, one rounding per operation, no contraction, except where f64 is named.  Candidates by
 * "Scan-to-map registration"'s rule: the stride, then the range gate.  Per candidate, with c, s, t' as there:
 *   q   = R_prior p_C
 *   p_M = ((c qx - s qy) + tx', (s qx + c qy) + ty', qz + tz')
 * Per candidate and submap k, in ASCENDING k:
 *   p_S = T_S_M,k p_M                          Eigen _transformVector, then + t
 *   the term is USABLE iff |p_S,a * block_size_inv| < 2^30 on every axis, all 8 neighbours exist in the submap's block
 *   table and are valid (ESDF observed != 0, TSDF weight > 0), and |r| < max_abs_distance_m, r the trilinear distance
 *   (special voxel values as in "Scan-to-map registration": a NaN, zero of either sign or negative TSDF weight is not
 *   > 0, a denormal or +inf one is; a NaN or infinite r has no term; -0.0 and denormal distances are ordinary values)
 *   g_S = (dD/d dl) * voxel_size_inv           the exact derivative of the interpolant, as there
 *   g_M = R(T_M_S,k) g_S                       the rotation alone (_transformVector), not renormalised
 *   J   = (g_Mx, g_My, g_Mz, g_Mx ((-s) qx - c qy) + g_My (c qx - s qy))
 * THE LOSS is Huber's, in f64 and in arithmetic alone (no log, no sqrt: every operation is IEEE-exact):
 *   rd = (double)r, a = (double)huber_delta_m;   |rd| <= a: w = 1, rho = rd rd;   else w = a / |rd|,
 *   rho = (2 a) |rd| - a a
 *   s0 += rho;   s[1 + k] += Jd[k] (w rd);   s[kl] += (w Jd[k]) Jd[l] in the pair order 00 01 02 03 11 12 13 22 23 33
 * With w = 1 (huber_delta_m = +inf, the default) these are "Scan-to-map registration"'s bits.  cost = 0.5 s0.  The
 * normal equations are the iteratively-reweighted-least-squares ones: there is NO second-order correction of the loss.
 * Three int64 counts: n_candidates; n_points_valid, the candidates with at least one usable term; n_terms.
 *
 * THE ORDER CONTRACT is "Scan-to-map registration"'s partition: candidate j to slot j / 1024, thread (j % 1024) % 256,
 * trip (j % 1024) / 256.  A thread adds its terms to 0.0 in ascending trip and within a trip in ascending k; then the
 * same wave tree, the waves in order, and the same fold of the slots' partials.  vgx_scan_registration_score_poses
 * applies the partition per pose with score_point_stride in place of point_stride.  A pose's result never depends on the
 * other poses of the call, on the device, or on which workgroup did the work.  No float atomics.
 *
 * _evaluate_map: two launches, one synchronisation.  out[15] = {s0, s[1..4], s[kl]}.
 * _score_poses: the cost alone at delta = 0 (c = 1, s = 0), for n_poses poses T_M_C [n_poses][7] (host): one upload of
 * the pose table, two launches and one synchronisation whatever n_poses.  For equal strides cost[m] is bit for bit
 * 0.5 out[0] of _evaluate_map(T_m, 0), and the counts are its counts.  Every output array is nullable.
 * _refine_map: "Scan-to-map registration"'s LOOP and OUTCOME with this evaluation; n_valid_first / n_valid_last carry
 * n_points_valid, and usable needs n_points_valid / n_candidates >= min_valid_ratio at the first and the last accepted
 * evaluation.
 * _localize: _score_poses; a pose is ELIGIBLE iff n_candidates > 0 and n_points_valid / n_candidates >= min_valid_ratio
 * (f64); score = cost / n_terms, one f64 division; best_index the lowest score, ties to the lowest index; then
 * _refine_map from T[best_index].  No eligible pose: VGX_OK, best_index = -1, a zeroed summary with usable = 0,
 * VGX_FAILURE / VGX_TERMINATION_TOO_FEW_POINTS, T_refined the bits of T[0], delta = 0, an empty history.  n_poses = 0
 * does that too, and then T_refined is not written.
 *
 * The calls run on the REGISTRATION side: the stream and the lock of vgx_submap_query, ordered behind
 * vgx_submap_generate_esdf.  A vgx_scan source is complete when its decode returned; a borrowed device array must be
 * ready with respect to the registration stream.  One call at a time per handle.
 *
 * Refused with VGX_ERR_INVALID, nothing written: NULL arguments; no map or no points set; a pose (of a submap, a prior,
 * a hypothesis) that is not finite or whose quaternion has | |q|^2 - 1 | > 1e-4; a delta that is not finite; a submap
 * of another context; submaps of different voxels_per_side; n_submaps < 0 or > 64; a layer value that is neither
 * VGX_EVAL_LAYER_ESDF nor _TSDF; huber_delta_m <= 0 or NaN; score_point_stride < 1; n_poses < 0; a layer not resident.
 * VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16; a launch of more than 2^31 - 1 workgroups (candidates / 1024,
 * times n_poses).  A refused _set_map leaves the map it found. */
typedef struct vgx_scan_map_config {
  int32_t layer;              /* VGX_EVAL_LAYER_ESDF */
  float huber_delta_m;        /* +inf: plain least squares */
  int32_t score_point_stride; /* 1: the stride of _score_poses (and of _localize's scoring) in place of point_stride */
  int32_t reserved;
} vgx_scan_map_config;
VGX_API void vgx_scan_map_config_default(vgx_scan_map_config* cfg);
/* cfg NULL: the defaults */
VGX_API int vgx_scan_registration_set_map(vgx_scan_registration reg, const vgx_scan_map_config* cfg, int32_t n_submaps,
                                          const vgx_submap* submaps, const float* T_M_S /* [n_submaps][7] */);
/* the three counts are nullable */
VGX_API int vgx_scan_registration_evaluate_map(vgx_scan_registration reg, const float T_M_C_prior[7], const double delta[4],
                                               double out[15], int64_t* n_terms, int64_t* n_points_valid,
                                               int64_t* n_candidates);
VGX_API int vgx_scan_registration_refine_map(vgx_scan_registration reg, const float T_M_C_prior[7],
                                             const vgx_pose_graph_options* options, float T_refined[7], double delta[4],
                                             vgx_scan_registration_summary* summary);
VGX_API int vgx_scan_registration_score_poses(vgx_scan_registration reg, int32_t n_poses,
                                              const float* T_M_C /* host [n_poses][7] */, double* cost, int64_t* n_terms,
                                              int64_t* n_points_valid, int64_t* n_candidates);
VGX_API int vgx_scan_registration_localize(vgx_scan_registration reg, int32_t n_poses, const float* T_M_C,
                                           const vgx_pose_graph_options* options, int32_t* best_index, float T_refined[7],
                                           double delta[4], vgx_scan_registration_summary* summary);

/* ---- View rendering: range images ray-marched out of a TSDF layer ------------ */
/* What the map looks like from a pose: per ray the range to the zero crossing of the trilinear TSDF, the surface point,
 * the gradient, the weight and the colour there -- the inverse of vgx_tsdf_integrate.  DEFINED HERE, not recalled:
 * voxblox has no ray caster over a layer (its RayCaster walks voxel indices for the integrators), DESIGN.md 27.  The
 * rules are built so that a numpy restatement reproduces every bit (tests/view_render_ref.py): f32, one rounding per
 * operation, no contraction, no transcendental or square root on the device, no float atomics.
 *
 * INPUTS.  A TSDF layer; a sensor pose T_L_C = {qw,qx,qy,qz, tx,ty,tz} (f32) in the layer's frame; n ray directions
 * dir [n][3] (f32) in the sensor frame.  The library NEVER normalises a direction: the ray parameter s is in units of
 * |dir| -- metres for unit directions -- and so are s_min, s_max, min_step, unknown_step and max_bracket.
 *
 * PER RAY.  o = t, d = R dir (Eigen _transformVector, the association of the map queries and scan registration).  A
 * ray whose dir has a non-finite component or is exactly (+-0, +-0, +-0) has status BAD and takes no sample.  Otherwise
 * s = s_min, have = false, and repeat:
 *   1. if !(s <= s_max): MISS.
 *   2. p_a = d_a * s + o_a (a multiply, then an add).
 *   3. the sample is INVALID unless |p_a * block_size_inv| < 2^30 on every axis (a non-finite p fails) and
 *      Interpolator<TsdfVoxel>::getVoxel(p, ., true) would succeed: all 8 neighbours' blocks exist, all 8 weights > 0.
 *   4. valid: D = the trilinear distance over the 8 neighbours (the interpolant of the map queries), and
 *        D > 0:        have = true; s0 = s; D0 = D; s = s + (D * step_scale > min_step ? D * step_scale : min_step)
 *        not (D > 0):  HIT when have and (s - s0) <= max_bracket, with s_hit = s0 + (s - s0) * (D0 / (D0 - D));
 *                      otherwise INSIDE -- the ray met the surface from behind, out of unknown space, or across a gap
 *                      too wide to interpolate over
 *      invalid: s = s + unknown_step; have, s0 and D0 are kept.
 * AT A HIT one more sample at p_hit = d * s_hit + o.  Valid: status HIT, gradient_a = (dD/d dl_a) * voxel_size_inv (the
 * exact derivative of the interpolant, "Scan-to-map registration"; layer frame, not normalised), weight = the
 * interpolated weight, rgba = the interpolated colour of the map products (per channel, clamped to [0, 255], truncated)
 * where the layer has colours, else 0.  Invalid: status HIT_UNSAMPLED, those three +0.  Either way range = s_hit and
 * points = dir_a * s_hit in the SENSOR frame (unit pinhole rays: points[..][2] is the z-depth).  Without a hit range and
 * points are +0: the integrators drop such points while min_ray_length_m > 0, and scan-to-map registration needs
 * min_range_m > 0 to do the same.  n_samples counts the positions sampled (step 2), valid or not, plus the one at the hit.
 * SPECIAL VOXEL VALUES fall under these comparisons as IEEE decides them.  A weight that is NaN, -0.0, +0.0 or negative
 * is not > 0 (the sample is invalid), a denormal or +inf weight is (the interpolated weight at the hit is then inf or NaN
 * by the interpolant's arithmetic).  A NaN D is "not (D > 0)": bracketed it is a hit whose range and points are NaN and
 * whose status is HIT_UNSAMPLED (the sample at a NaN position is invalid), unbracketed it is INSIDE.  D = +inf makes
 * s = +inf: MISS.  D = -inf bracketed gives s_hit = s0 exactly, the hit at the last positive sample; unbracketed INSIDE.
 * -0.0 is "not (D > 0)"; a denormal D > 0 is a positive distance (nothing is flushed).
 *
 * s_max / min(min_step, unknown_step) <= 65536 bounds the loop and keeps every increment far above one ulp of s.
 * s_max, min_step, unknown_step and max_bracket have NO default (0 is refused); a starting point is the reach wanted,
 * voxel_size / 4, voxel_size and the layer's truncation distance.
 *
 * image_width > 0 only changes which lane takes which ray (ray i is pixel (i % image_width, i / image_width); a wave
 * takes an 8 x 8 tile, so its rays stay in neighbouring voxels); the results are the same bits.  The counts are int64
 * sums (integer atomics).  A vgx_view owns the device outputs (range and status always, the others by flag), grown on
 * demand; its device pointers hold until a later render grows them or the view is destroyed.  points plugs into
 * vgx_scan_registration_set_points_device and vgx_tsdf_integrate_device as it stands.
 *
 * vgx_tsdf_layer_render_view (the active layer, the projected map) runs on the TSDF stream under the integrators' lock,
 * ordered behind every scan already queued; vgx_submap_render_view reads a finished submap's raw TSDF layer on the
 * registration stream under its lock, the pose in the submap's frame.  One launch, one 64-byte copy of the counts and
 * one host synchronisation per call; the host-pointer forms copy the directions first.  One call at a time per handle.
 *
 * Refused with VGX_ERR_INVALID, nothing written: NULL arguments; a layer or submap of another context; n < 0; a pose
 * that is not finite or whose quaternion has | |q|^2 - 1 | > 1e-4; a submap whose raw layers were released; at creation
 * any field that is not finite, s_min < 0, s_min > s_max, step_scale <= 0, s_max / min_step / unknown_step /
 * max_bracket <= 0, s_max / min(min_step, unknown_step) > 65536, image_width < 0, unknown flag bits;
 * vgx_view_download of an output the flags do not hold.  VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16; more
 * rays than one launch takes.  n = 0: VGX_OK, the view then holds no ray. */
#define VGX_VIEW_MISS 0
#define VGX_VIEW_HIT 1
#define VGX_VIEW_INSIDE 2
#define VGX_VIEW_BAD 3
#define VGX_VIEW_HIT_UNSAMPLED 4
#define VGX_VIEW_POINTS 1
#define VGX_VIEW_GRADIENT 2
#define VGX_VIEW_WEIGHT 4
#define VGX_VIEW_RGBA 8
#define VGX_VIEW_N_SAMPLES 16
#define VGX_VIEW_ALL 31
typedef struct vgx_view_s* vgx_view;
typedef struct vgx_view_config {
  float s_min;         /* 0 */
  float s_max;         /* NO default (0: refused) */
  float step_scale;    /* 0.75 */
  float min_step;      /* NO default: e.g. voxel_size / 4 */
  float unknown_step;  /* NO default: e.g. voxel_size */
  float max_bracket;   /* NO default: e.g. the layer's truncation distance */
  int32_t image_width; /* 0: rays map to lanes by index */
  int32_t flags;       /* VGX_VIEW_POINTS; which optional outputs the view holds */
} vgx_view_config;
typedef struct vgx_view_counts {
  int64_t n_rays, n_hit, n_hit_unsampled, n_miss, n_inside, n_bad;
  int64_t n_samples;
  int64_t reserved;
} vgx_view_counts;
VGX_API void vgx_view_config_default(vgx_view_config* cfg);
/* host only: VGX_OK, or VGX_ERR_INVALID where vgx_view_create would refuse the config */
VGX_API int vgx_view_config_check(const vgx_view_config* cfg);
VGX_API int vgx_view_create(vgx_ctx ctx, const vgx_view_config* cfg, vgx_view* out);
VGX_API int vgx_view_destroy(vgx_view view);
/* the counts of the view held now (all zero before the first render) */
VGX_API int vgx_view_stats(vgx_view view, vgx_view_counts* counts);
/* every array nullable; range [n] f32, status [n] u8, points / gradient [n][3] f32, weight [n] f32, rgba [n] u32 (bytes
 * r g b a, r lowest), n_samples [n] i32, n = counts.n_rays */
VGX_API int vgx_view_download(vgx_view view, float* range, uint8_t* status, float* points, float* gradient, float* weight,
                              uint32_t* rgba, int32_t* n_samples);
/* NULL for an output the view does not hold, and for all of them while it holds no ray */
VGX_API int vgx_view_device_pointers(vgx_view view, const float** range, const uint8_t** status, const float** points,
                                     const float** gradient, const float** weight, const uint32_t** rgba,
                                     const int32_t** n_samples);
VGX_API int vgx_tsdf_layer_render_view(vgx_tsdf_layer layer, vgx_view view, const float T_L_C[7], int64_t n,
                                       const float* dirs /* host [n][3] */);
VGX_API int vgx_tsdf_layer_render_view_device(vgx_tsdf_layer layer, vgx_view view, const float T_L_C[7], int64_t n,
                                              const void* d_dirs /* f32 [n][3], ready with respect to the TSDF stream */);
VGX_API int vgx_submap_render_view(vgx_submap submap, vgx_view view, const float T_S_C[7], int64_t n, const float* dirs);
VGX_API int vgx_submap_render_view_device(vgx_submap submap, vgx_view view, const float T_S_C[7], int64_t n,
                                          const void* d_dirs /* ready with respect to the registration stream */);
/* Host-only ray helpers: unit directions computed in f64 and rounded to f32 once, row-major dirs[row][col][3].
 * pinhole: ((u - cx) / fx, (v - cy) / fy, 1) normalised, u the column, v the row.
 * lidar:   az = -pi + azimuth_offset + col * 2 pi / width, el = elevation_min + row * (elevation_max - elevation_min) /
 *          (height - 1) (height 1: elevation_min), dir = (cos el cos az, cos el sin az, sin el).
 * VGX_ERR_INVALID: width or height < 1, NULL dirs, a parameter that is not finite, fx or fy zero. */
VGX_API int vgx_view_rays_pinhole(int32_t width, int32_t height, double fx, double fy, double cx, double cy, float* dirs);
VGX_API int vgx_view_rays_lidar(int32_t width, int32_t height, double elevation_min, double elevation_max,
                                double azimuth_offset, float* dirs);

/* ---- Planar map: the 2D occupancy and distance grid of a layer's height band -------- */
/* What a 2D planner takes: the voxels of a layer between two heights collapsed along z into a grid of cells -- state,
 * nav_msgs/OccupancyGrid occupancy, clearance, obstacle height -- and the exact planar Euclidean distance to the nearest
 * obstacle cell, clipped.  Every submap frame and the mission frame are gravity-aligned (the pose graph is 4-DoF), so a
 * band of z rows is well defined in any layer and nothing is resampled.  Sources: a vgx_tsdf_layer (the active submap
 * or the projected map) and a finished submap's raw TSDF or ESDF layer.
 * Rules (what the kernels, vgx_planar.hip, and tests/planar_map_ref.py both follow; f32 with no contraction unless
 * marked int):
 *   cell       global voxel index on x and y, ix = block_x * vps + local_x (int32).  The grid is row-major, x fastest:
 *              cell = (iy - y0) * W + (ix - x0), OccupancyGrid's order, with its origin at the corner (x0 * voxel_size,
 *              y0 * voxel_size).  A layer whose block table reaches block indices that overflow ix: VGX_ERR_INVALID.
 *   observed   the clouds' rule: ESDF observed != 0; TSDF weight > min_weight, strictly (a NaN weight is not observed).
 *   band       a voxel row with centre cz = voxel_centre((float)bz * block_size, lz, voxel_size) -- block_size =
 *              (float)vps * voxel_size, the helper that of every other product -- is in the band iff z_min <= cz &&
 *              cz <= z_max.  A block none of whose rows passes this very comparison is skipped unread.
 *   voxel      occupied_v: in the band, observed, d <= occupied_distance.  free_v: in the band, observed,
 *              d > occupied_distance.  A NaN distance is neither; +-inf classify by the comparison.
 *   column     a cell's voxels are walked in ascending global z; missing blocks are skipped.  n_occ, n_free: int32.
 *   state      u8: 2 (occupied) if n_occ >= 1, else 1 (free) if n_free >= min_free_voxels, else 0 (unknown).
 *   clearance  f32: the smallest d over the classified voxels; it starts at the first one and is replaced only when
 *              d < current, strictly, so ties (+-0) are decided by z order.  +0.0f where state is 0 -- also where fewer
 *              than min_free_voxels free voxels were seen.
 *   height     f32: cz of the highest occupied_v; +0.0f where state != 2.
 *   occupancy  i8: -1 / 0 / 100 for state 0 / 1 / 2.
 *   box        use_box = 0: the x/y extent, in whole blocks, of the allocated blocks that have at least one row in the
 *              band; none: W = H = 0 and VGX_OK.  use_box = 1: cell_min[2], cell_dim[2] in global voxel indices, not
 *              necessarily block-aligned (a rolling window); cells outside the layer are unknown.  cell_dim >= 0 and
 *              cell_min + cell_dim <= 2^31 - 1; W * H <= 2^28, else VGX_ERR_INVALID.
 *   distance   f32 per cell.  Obstacle cells: state 2, and state 0 when unknown_is_obstacle != 0.  R =
 *              (int)ceil((double)max_distance_m / (double)voxel_size), on the host; max_distance_m finite and > 0 and
 *              R <= 2048, so that 2 R^2 < 2^24 and (float)d2 is exact.  Row pass (int): g[y][x] = the smallest |x - x'|
 *              over the obstacle cells of row y with |x - x'| <= R, or none.  Column pass (int): d2 = min over
 *              |dy| <= R, row y + dy inside the grid, g[y + dy][x] not none, of dy * dy + g * g.  Then m =
 *              sqrtf((float)d2) * voxel_size and distance = m < max_distance_m ? m : max_distance_m; max_distance_m
 *              where nothing was found; 0 on obstacle cells.  Nothing outside the box is an obstacle.  A candidate
 *              outside the square window is at least (R + 1) * voxel_size away and clips anyway: the result is the
 *              exact Euclidean distance transform, clipped.
 *   totals     the number of cells in each state, counts[3] int64, indexed by state.
 * The handle is reused from call to call: its device buffers grow on demand; one call at a time per handle.
 * Refused with VGX_ERR_INVALID before anything is written, the map keeping what it held (vgx_last_error says which): a
 * NULL source, map or cfg (there is no default band), a map of another context, z_min, z_max or occupied_distance not
 * finite, z_min > z_max, a min_weight that is negative or not finite, min_free_voxels < 1, max_distance_m not finite or
 * <= 0 or R > 2048, a bad box, a submap layer that is not resident in raw form, a layer value that is neither
 * VGX_EVAL_LAYER_ESDF nor _TSDF.  VGX_ERR_UNSUPPORTED: voxels_per_side other than 8 or 16.  Out of device memory:
 * VGX_ERR_NOMEM, and the map then holds 0 cells.
 * Passes: [the box: one kernel over the block slots, integer min / max] -- gather (one lane per cell walks the band's z
 * blocks through the layer's dense block table; no atomics on cells, integer atomics for the three totals) -- row pass
 * -- column pass: a fixed number of launches whatever the size.  Two host synchronisations (the box, then the end with
 * the totals); one with use_box.  vgx_submap_layer_planar_map runs on the registration stream under the registration
 * lock, behind vgx_submap_generate_esdf; vgx_tsdf_layer_planar_map on the TSDF stream under the TSDF lock, behind the
 * scans and merges already queued.  Both return with the map complete. */
typedef struct vgx_planar_map_config {
  float z_min, z_max;          /* NaN: the band has no default and must be set (metres, the layer's frame) */
  float occupied_distance;     /* 0: at or behind the surface */
  float min_weight;            /* 1e-3, TSDF sources only */
  int32_t min_free_voxels;     /* 1 */
  int32_t unknown_is_obstacle; /* 0 */
  float max_distance_m;        /* 2 */
  int32_t use_box;             /* 0 */
  int32_t cell_min[2];         /* 0, 0 (use_box: x0, y0, global voxel indices) */
  int32_t cell_dim[2];         /* 0, 0 (use_box: W, H) */
} vgx_planar_map_config;
typedef struct vgx_planar_map_s* vgx_planar_map;
/* fills all but the band: z_min = z_max = NaN, so that an unset band is refused */
VGX_API void vgx_planar_map_config_default(vgx_planar_map_config* cfg);
VGX_API int vgx_planar_map_create(vgx_ctx ctx, vgx_planar_map* out);
VGX_API int vgx_planar_map_destroy(vgx_planar_map map);
/* a vgx_tsdf_layer: the active submap or the projected map */
VGX_API int vgx_tsdf_layer_planar_map(vgx_tsdf_layer layer, const vgx_planar_map_config* cfg, vgx_planar_map map);
/* a finished submap's raw layer: layer = VGX_EVAL_LAYER_ESDF / VGX_EVAL_LAYER_TSDF */
VGX_API int vgx_submap_layer_planar_map(vgx_submap submap, int32_t layer, const vgx_planar_map_config* cfg,
                                        vgx_planar_map map);
/* any pointer may be NULL; cell_min = {x0, y0}, cell_dim = {W, H}, counts indexed by state */
VGX_API int vgx_planar_map_stats(vgx_planar_map map, int32_t cell_min[2], int32_t cell_dim[2], float* voxel_size,
                                 int64_t counts[3]);
/* A measuring aid, off by default: with enable != 0 the producing calls record events between their launches, and
 * vgx_planar_map_pass_ms returns the device time of the last producing call by pass (milliseconds): ms[0] the box kernel
 * (0 with use_box, or where no block has a row in the band), ms[1] gather, ms[2] row pass, ms[3] column pass; all 0 for a
 * map of 0 cells or while timing is off.  What profiles/planar_map_bench.py reports. */
VGX_API int vgx_planar_map_set_timing(vgx_planar_map map, int32_t enable);
VGX_API int vgx_planar_map_pass_ms(vgx_planar_map map, float ms[4]);
/* state [H][W] u8, occupancy [H][W] i8, clearance, height, distance [H][W] f32; any may be NULL */
VGX_API int vgx_planar_map_download(vgx_planar_map map, uint8_t* state, int8_t* occupancy, float* clearance, float* height,
                                    float* distance);
/* DEVICE pointers to the same five arrays (NULL while the map holds 0 cells); valid until the next producing call on
 * the handle or its destruction.  Any may be NULL. */
VGX_API int vgx_planar_map_device_pointers(vgx_planar_map map, const uint8_t** state, const int8_t** occupancy,
                                           const float** clearance, const float** height, const float** distance);

/* ---- Elevation map: 2.5D surface height, slope, step and traversability of a layer's height band -------- */
/* What a legged or rough-terrain planner takes: per cell of the planar map's grid the height of the surface to sub-voxel
 * accuracy, the headroom above it, the step height and support of its neighbourhood, the surface gradient and slope, a
 * traversability class, and the exact planar Euclidean distance to the nearest non-traversable cell, clipped.  The
 * formulation is this library's own: neither voxgraph nor voxblox builds such a grid.  Sources: a vgx_tsdf_layer (the
 * active submap or the projected map) and a finished submap's raw TSDF or ESDF layer.
 * Rules (what the kernels, vgx_elevation.hip, and tests/elevation_map_ref.py both follow; f32 with no contraction
 * unless marked int):
 *   shared     cell, grid order, box, observed and band are exactly the planar map's rules above: the global voxel index
 *              and x fastest; the default box from the blocks with a row in the band, or a rolling window; W * H <= 2^28;
 *              the voxel_centre helper and z_min <= cz && cz <= z_max.
 *   column     walk a cell's voxel rows in descending global z, from the top row of the band to the bottom one; rows
 *              that belong to a missing block are included.  A voxel is classified when it is in the band, observed,
 *              and its distance d is not NaN; it is free_v when d > 0.0f, else solid_v.  Carry run (int), the number of
 *              consecutive classified free_v voxels immediately above the current row; any row that is unclassified,
 *              solid_v, missing or out of band resets run to 0.  A crossing is a solid_v voxel l met with run >= 1.
 *              Then d_u is the distance of the voxel directly above, t = (-d_l) / (d_u - d_l), and if
 *              !(t >= 0.0f && t <= 1.0f) then t = 0.5f (that case arises from +-inf operands).  h = cz_l + t *
 *              voxel_size and headroom = run.  n_free, n_solid and crossings are int32 counts; crossings is stored as
 *              u8, saturating at 255.  Adjacency never skips a row: a missing block between two voxels is not a
 *              crossing; a pair that straddles a z block boundary is one.
 *   outputs    pick chooses the first crossing met (0: the highest) or the last one (1: the lowest).  state u8: 1 =
 *              surface (at least one crossing); 3 = blocked (no crossing, n_solid >= 1); 2 = hole (no crossing, n_solid
 *              == 0, n_free >= min_free_voxels); 0 = unknown (everything else).  height f32: h of the chosen crossing,
 *              +0.0f where state is not 1.  headroom i32: voxels, 0 where state is not 1.  crossings u8.
 *   step       the window is the cells within Chebyshev distance step_radius_cells (0..64) inside the box.  support
 *              (u16) is the number of state-1 cells in the window, the cell itself included; step = max(height) -
 *              min(height) over those cells.  Both are 0 where the cell's own state is not 1.  Max and min are exact,
 *              computed separably: a row pass, then a column pass -- O(radius) per cell.
 *   gradient   for a cell in state 1 (any other cell has both axes undefined).  On x, with h_r and h_l the heights of
 *              the x + 1 and x - 1 cells where they are inside the box and in state 1: both: gx = (h_r - h_l) / (2.0f *
 *              voxel_size); only right: (h_r - h) / voxel_size; only left: (h - h_l) / voxel_size; neither: the axis is
 *              undefined.  gy is formed likewise.  slope = sqrtf(gx * gx + gy * gy) when both axes are defined;
 *              otherwise the slope is undefined, stored as +0.0f, with slope_valid (u8) = 0.  grad is stored as f32[2],
 *              zeros where the slope is undefined.
 *   class      u8, decided in this order.  1. state 0 gives class 0.  2. state 3 gives class 2.  3. state 2 gives class
 *              2 if hole_is_obstacle, else 0.  4. state 1: headroom < min_headroom_voxels gives 2; else !slope_valid ||
 *              support < min_support gives 0; else slope > max_slope || step > max_step_m gives 2; else 1.
 *              (0 unknown, 1 traversable, 2 not traversable.)
 *   distance   f32, to the nearest obstacle cell: class 2, and also class 0 when unknown_is_obstacle.  The planar map's
 *              rule word for word: the same R, with R <= 2048; an integer row pass and an integer column pass;
 *              sqrtf((float)d2) * voxel_size; the clip; nothing outside the box is an obstacle.
 *   totals     the number of cells in each state, state_counts[4], and in each class, class_counts[3]; int64.
 * The handle is reused from call to call: its device buffers grow on demand; one call at a time per handle.
 * Refused with VGX_ERR_INVALID before anything is written, the map keeping what it held (vgx_last_error says which): the
 * planar map's list -- a NULL source, map or cfg (there is no default band), a map of another context, z_min or z_max
 * not finite, z_min > z_max, a min_weight that is negative or not finite, min_free_voxels < 1, max_distance_m not finite
 * or <= 0 or R > 2048, a bad box, a submap layer that is not resident in raw form, a layer value that is neither
 * VGX_EVAL_LAYER_ESDF nor _TSDF -- and pick not 0 or 1, step_radius_cells outside 0..64, min_support < 1,
 * min_headroom_voxels < 1, max_slope or max_step_m NaN or negative.  VGX_ERR_UNSUPPORTED: voxels_per_side other than 8
 * or 16.  Out of device memory: VGX_ERR_NOMEM, and the map then holds 0 cells.
 * Passes: [the box, the planar map's kernel] -- gather (one lane per cell walks the band's z blocks downwards through
 * the dense block table; no atomics on cells, integer atomics for the state totals) -- step row pass -- step column pass
 * with the gradient, slope and class (integer atomics for the class totals) -- distance row pass -- distance column pass
 * (the planar map's two kernels over the class): a fixed number of launches whatever the size.  Two host
 * synchronisations (the box, then the end with the totals); one with use_box.  No float atomics.
 * vgx_submap_layer_elevation_map runs on the registration stream under the registration lock;
 * vgx_tsdf_layer_elevation_map on the TSDF stream under the TSDF lock, behind the scans and merges already queued.  Both
 * return with the map complete. */
typedef struct vgx_elevation_map_config {
  float z_min, z_max;           /* NaN: the band has no default and must be set (metres, the layer's frame) */
  float min_weight;             /* 1e-3, TSDF sources only */
  int32_t min_free_voxels;      /* 1 */
  int32_t pick;                 /* 0 = the highest crossing, 1 = the lowest */
  int32_t step_radius_cells;    /* 1 (0..64) */
  int32_t min_support;          /* 1 */
  float max_slope;              /* 1.0, rise over run */
  float max_step_m;             /* 0.2 */
  int32_t min_headroom_voxels;  /* 1 */
  int32_t hole_is_obstacle;     /* 1 */
  int32_t unknown_is_obstacle;  /* 0 */
  float max_distance_m;         /* 2 */
  int32_t use_box;              /* 0 */
  int32_t cell_min[2];          /* 0, 0 (use_box: x0, y0, global voxel indices) */
  int32_t cell_dim[2];          /* 0, 0 (use_box: W, H) */
} vgx_elevation_map_config;
typedef struct vgx_elevation_map_s* vgx_elevation_map;
/* fills all but the band: z_min = z_max = NaN, so that an unset band is refused */
VGX_API void vgx_elevation_map_config_default(vgx_elevation_map_config* cfg);
VGX_API int vgx_elevation_map_create(vgx_ctx ctx, vgx_elevation_map* out);
VGX_API int vgx_elevation_map_destroy(vgx_elevation_map map);
/* a vgx_tsdf_layer: the active submap or the projected map */
VGX_API int vgx_tsdf_layer_elevation_map(vgx_tsdf_layer layer, const vgx_elevation_map_config* cfg, vgx_elevation_map map);
/* a finished submap's raw layer: layer = VGX_EVAL_LAYER_ESDF / VGX_EVAL_LAYER_TSDF */
VGX_API int vgx_submap_layer_elevation_map(vgx_submap submap, int32_t layer, const vgx_elevation_map_config* cfg,
                                           vgx_elevation_map map);
/* any pointer may be NULL; cell_min = {x0, y0}, cell_dim = {W, H}, state_counts indexed by state, class_counts by class */
VGX_API int vgx_elevation_map_stats(vgx_elevation_map map, int32_t cell_min[2], int32_t cell_dim[2], float* voxel_size,
                                    int64_t state_counts[4], int64_t class_counts[3]);
/* A measuring aid, off by default (no event is made or recorded while off): with enable != 0 the producing calls record
 * events between their launches, and vgx_elevation_map_pass_ms returns the device time of the last producing call by
 * pass (milliseconds): ms[0] the box kernel (0 with use_box, or where no block has a row in the band), ms[1] gather,
 * ms[2] step row pass, ms[3] step column pass with slope and class, ms[4] distance row pass, ms[5] distance column pass;
 * all 0 for a map of 0 cells or while timing is off.  What profiles/elevation_map_bench.py reports. */
VGX_API int vgx_elevation_map_set_timing(vgx_elevation_map map, int32_t enable);
VGX_API int vgx_elevation_map_pass_ms(vgx_elevation_map map, float ms[6]);
/* state, crossings, slope_valid, cls [H][W] u8; headroom [H][W] i32; support [H][W] u16; height, step, slope, distance
 * [H][W] f32; grad [H][W][2] f32 (gx, gy); any may be NULL */
VGX_API int vgx_elevation_map_download(vgx_elevation_map map, uint8_t* state, float* height, int32_t* headroom,
                                       uint8_t* crossings, uint16_t* support, float* step, float* grad, float* slope,
                                       uint8_t* slope_valid, uint8_t* cls, float* distance);
/* DEVICE pointers to the same eleven arrays (NULL while the map holds 0 cells); valid until the next producing call on
 * the handle or its destruction.  Any may be NULL. */
VGX_API int vgx_elevation_map_device_pointers(vgx_elevation_map map, const uint8_t** state, const float** height,
                                              const int32_t** headroom, const uint8_t** crossings, const uint16_t** support,
                                              const float** step, const float** grad, const float** slope,
                                              const uint8_t** slope_valid, const uint8_t** cls, const float** distance);

#ifdef __cplusplus
}
#endif
#endif /* VOXGRAPH_AMD_H_ */
