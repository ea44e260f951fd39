/*
 * mpas_dycore.h -- C ABI of the MI355X-native MPAS-Atmosphere dycore.
 *
 * This is the drop-in boundary behind the reference's Fortran operator API
 * (module atm_time_integration, src/core_atmosphere/dynamics/
 * mpas_atm_time_integration.F).  A Fortran shim module named
 * atm_time_integration keeps the reference's public
 * routines and binds these entry points with iso_c_binding:
 *
 *   atm_timestep(domain, dt, nowTime, itimestep)      mpas_atm_time_integration.F:87
 *       -> mpas_dyc_timestep                          (atm_srk3, :142-1796)
 *   atm_init_coupled_diagnostics(state, 1, diag, ...) mpas_atm_time_integration.F:5825
 *   atm_compute_solve_diagnostics(dt, state, 1, ...)  mpas_atm_time_integration.F:5419
 *       -> mpas_dyc_init_diagnostics                  (called at mpas_atm_core.F:390,399)
 *   mpas_pool_shift_time_levels(state)                mpas_pool_routines.F:5541
 *       -> mpas_dyc_shift_time_levels                 (called at mpas_atm_core.F:671)
 *   mpas_pool_get_array(pool, name, ptr[, timeLevel])  mpas_pool_routines.F:4282
 *       -> mpas_dyc_set_field / mpas_dyc_get_field    (pool-owned host memory <-> HBM)
 *
 * Conventions (match what the Fortran pools hold, so the shim passes pool
 * pointers unchanged):
 *   - real fields are fp64 Fortran memory images including the garbage slot:
 *     u(nVertLevels, nEdges+1), w(nVertLevels+1, nCells+1),
 *     scalars(num_scalars, nVertLevels, nCells+1), zb_cell(nVertLevels+1, maxEdges, nCells+1) ...
 *   - integer fields are int32 with MPAS 1-based indices (n+1 = garbage slot);
 *   - time_level is 1 or 2 for the state pool (ignored otherwise).
 * All functions return 0 on success and a negative MPAS_DYC_E* code on error
 * (the shim maps non-zero to mpas_log_write(..., MPAS_LOG_CRIT), which is how
 * the reference reports fatal errors, mpas_log.F:612).  No torch types, no
 * C++ types: plain pointers and sizes.
 */
#ifndef MPAS_DYCORE_H
#define MPAS_DYCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPAS_DYC_OK 0
#define MPAS_DYC_EINVAL -1    /* bad argument / unknown field / size mismatch */
#define MPAS_DYC_EHIP -2      /* HIP runtime error */
#define MPAS_DYC_ESTATE -3    /* call out of sequence */
#define MPAS_DYC_ECOMM -4     /* halo exchange failure */

/* nVertLevels: 4..MPAS_DYC_MAX_LEVELS.  Up to MPAS_DYC_MAX_LEVELS_WAVE a column is one 64-lane
 * wavefront (lane = level), or half of one in the pair layout (two levels per lane); up to
 * MPAS_DYC_MAX_LEVELS_WIDE the pair-layout kernels give a whole wavefront to one column (two levels
 * per lane) and the per-cell kernels one 128-lane workgroup, whose cross-level moves go through LDS;
 * above, every kernel runs one column per workgroup of the next multiple of 64 lanes above the
 * column's K + 1 levels (192, 256, 320, 384, 448 or 512; MPAS_DYCORE_WIDE_TIGHT=0: 256 up to
 * MPAS_DYC_MAX_LEVELS_256, 512 above); the pair-layout kernels there keep two levels per lane
 * over the first 128, 192 or 256 lanes of the workgroup.  Regional LBCs run at every
 * nVertLevels (they need the pair layout, which every build has). */
#define MPAS_DYC_MAX_LEVELS_WAVE 63
#define MPAS_DYC_MAX_LEVELS_WIDE 127
#define MPAS_DYC_MAX_LEVELS_192 191
#define MPAS_DYC_MAX_LEVELS_256 255
#define MPAS_DYC_MAX_LEVELS 511

typedef struct mpas_dyc_ctx mpas_dyc_ctx;

/* Registry.xml dims (8-46) for one block; *Solve = owned counts (mpas_block_creator.F). */
typedef struct {
  int32_t nCells, nEdges, nVertices, nVertLevels, maxEdges, maxEdges2, num_scalars;
  int32_t nCellsSolve, nEdgesSolve, nVerticesSolve;
  int32_t moist_start, moist_end; /* 1-based, as in the state pool */
  int32_t index_qv;               /* 1-based */
} mpas_dyc_dims;

/* nhyd_model namelist (Registry.xml:56-290).  Logicals as int 0/1;
 * config_horiz_mixing: 1 = "2d_smagorinsky", 0 = "2d_fixed". */
typedef struct {
  int32_t config_time_integration_order, config_number_of_sub_steps, config_dynamics_split_steps;
  int32_t config_number_rayleigh_damp_u_levels;
  int32_t config_split_dynamics_transport, config_scalar_advection, config_positive_definite;
  int32_t config_monotonic, config_mix_full, config_rayleigh_damp_u, config_horiz_mixing;
  double config_h_mom_eddy_visc2, config_h_mom_eddy_visc4, config_v_mom_eddy_visc2;
  double config_h_theta_eddy_visc2, config_h_theta_eddy_visc4, config_v_theta_eddy_visc2;
  double config_len_disp, config_visc4_2dsmag, config_del4u_div_factor, config_coef_3rd_order;
  double config_smagorinsky_coef, config_epssm, config_smdiv, config_apvm_upwinding;
  double config_mpas_cam_coef, config_rayleigh_damp_u_timescale_days;
} mpas_dyc_config;

/* Create a dycore context on HIP device `device` (-1 = current); allocates all
 * device fields (mesh, state x2 time levels, diag, tend, module scratch).
 * device = MPAS_DYC_HOST_ONLY: a planner-only context (see mpas_dyc_plan_exchanges). */
int mpas_dyc_create(const mpas_dyc_dims* dims, const mpas_dyc_config* cfg, int device, mpas_dyc_ctx** out);
void mpas_dyc_destroy(mpas_dyc_ctx* ctx);
const char* mpas_dyc_last_error(const mpas_dyc_ctx* ctx);

/* Host <-> device copy of one named pool field (pool: "mesh","state","diag","tend",
 * "tend_physics", "lbc", "tend_iau" -- see mpas_dyc_set_iau; scalars 0-d fields cf1/cf2/cf3 take 8
 * bytes). nbytes must match.  diag.w_velocity_max / wind_speed_level1_max / updraft_helicity_max: see
 * mpas_dyc_set_diag_update.  "diag_physics" rainnc / rainncv / precipw / i_rainnc, diag.surface_pressure,
 * tend.tend_sfc_pressure: see mpas_dyc_set_microphysics. */
int mpas_dyc_set_field(mpas_dyc_ctx* ctx, const char* pool, const char* name, int32_t time_level,
                       const void* host, int64_t nbytes);
int mpas_dyc_get_field(mpas_dyc_ctx* ctx, const char* pool, const char* name, int32_t time_level,
                       void* host, int64_t nbytes);
/* Size in bytes of a field's Fortran memory image (0 if unknown). */
int64_t mpas_dyc_field_bytes(const mpas_dyc_ctx* ctx, const char* pool, const char* name);
/* Raw device pointer of a field (for zero-copy use from torch / RCCL); NULL if unknown.
 * Device layout = the Fortran image, except scalars / scalars_tend, which are
 * scalar-major [num_scalars][n+1][nVertLevels] in HBM (set/get transpose them).
 * A pointer is valid until the next mpas_dyc_timestep / mpas_dyc_shift_time_levels: the step
 * rotates buffers instead of copying them, so re-query it after every step for
 *   - diag.ru, ru_save, rw, rw_save, rtheta_p, rtheta_p_save, rho_p, rho_p_save (the _save
 *     copies of atm_rk_integration_setup / atm_rk_dynamics_substep_finish, 1847-1850, 6051-6054,
 *     are buffer trades),
 *   - state.theta_m (theta_m_1 = theta_m_2 at every substep end, 6058, is a trade of its two
 *     time levels), and every state field's time levels across mpas_dyc_shift_time_levels.
 * The maxEdges / maxEdges2-strided mesh fields (edgesOnCell, cellsOnCell, verticesOnCell,
 * kiteForCell, edgesOnCell_sign, defc_a, defc_b, coeffs_reconstruct, zb_cell, zb3_cell,
 * edgesOnEdge, weightsOnEdge) return their image at the declared maxEdges; the kernels read a
 * copy at the mesh's actual cell degree (mpas_dyc_block_layout), so change them through
 * mpas_dyc_set_field, not through this pointer. */
void* mpas_dyc_field_device_ptr(mpas_dyc_ctx* ctx, const char* pool, const char* name, int32_t time_level);

/* atm_init_coupled_diagnostics + atm_compute_solve_diagnostics on time level 1
 * (model init, mpas_atm_core.F:387-404). */
int mpas_dyc_init_diagnostics(mpas_dyc_ctx* ctx, double dt);
/* The same model init for a restart (config_do_restart, mpas_atm_core.F:387-404): only
 * atm_compute_solve_diagnostics (with the init exchanges), on a state whose coupled fields
 * (theta_m, rho_zz, rho_p, rtheta_p, exner, pressure_p, ru, rw, ...) the host has set. */
int mpas_dyc_solve_diagnostics(mpas_dyc_ctx* ctx, double dt);
/* atm_timestep -> atm_srk3: advance time level 1 to time level 2 by dt. Asynchronous.  itimestep is
 * the model's step counter (1 = the first step of the run): with mpas_dyc_set_iau on it decides whether
 * the step is inside the IAU window; nothing else reads it. */
int mpas_dyc_timestep(mpas_dyc_ctx* ctx, double dt, int32_t itimestep);
/* mpas_pool_shift_time_levels(state): swap time levels 1 and 2 (pointer swap).  Between steps, only
 * time level 1 (the state the last step produced) is defined for u and w: the step does not copy
 * u_2 / w_2 into time level 1 at its substep ends (6060-6061), because nothing reads them before
 * the next step's atm_rk_integration_setup overwrites that buffer (1852-1853).  Read u and w at
 * time level 1 after the shift. */
int mpas_dyc_shift_time_levels(mpas_dyc_ctx* ctx);
/* Block until all queued device work of the context is complete. */
int mpas_dyc_synchronize(mpas_dyc_ctx* ctx);
/* Physics coupling (the reference built with -DDO_PHYSICS, mpas_atm_time_integration.F:424-449,
 * 1610-1648, 3437, 3743).  With MPAS_DYC_PHYSICS_TENDENCIES the host (the physics package's
 * physics_get_tend, mpas_atmphys_todynamics.F:59) supplies, before each mpas_dyc_timestep,
 *   tend_physics.tend_ru_physics (K, nEdges+1), tend_physics.tend_rtheta_physics and
 *   tend_physics.tend_rho_physics (K, nCells+1), and tend.scalars_tend (ns, K, nCells+1);
 * the step adds them where the reference does (tend_u, tend_theta, tend_rho; the scalar
 * transport's scalar_tend_save / scalar_tend), and at its end sets negative scalars of time
 * level 2 to zero (1645-1646).  MPAS_DYC_PHYSICS_RQVDYNTEN also computes tend_physics.rqvdynten
 * (1629-1643; config_convection_scheme cu_grell_freitas, cu_tiedtke or cu_ntiedtke).  The
 * microphysics driver (1650-1660) stays with the host, after the step. */
#define MPAS_DYC_PHYSICS_TENDENCIES 1
#define MPAS_DYC_PHYSICS_RQVDYNTEN 2
/* MPAS_DYC_PHYSICS_MICROPHYSICS: the host runs driver_microphysics (1650-1660) after each
 * mpas_dyc_timestep, on time level 2 of the step (uploading what it changes: theta_m and scalars of
 * time level 2, rtheta_p, exner, pressure_p, rt_diabatic_tend), and then calls mpas_dyc_finish_step,
 * which runs what follows the microphysics in atm_srk3: the regional reset of the specified zone
 * (1672-1790, config_apply_lbcs) and summarize_timestep's reductions (1794).  Without this flag
 * mpas_dyc_timestep runs them itself and mpas_dyc_finish_step does nothing.
 * MPAS_DYC_EINVAL: unknown bits, MPAS_DYC_PHYSICS_RQVDYNTEN without MPAS_DYC_PHYSICS_TENDENCIES.
 * MPAS_DYC_ESTATE: MPAS_DYC_PHYSICS_MICROPHYSICS with mpas_dyc_set_microphysics on, or
 * MPAS_DYC_PHYSICS_TENDENCIES with mpas_dyc_set_todynamics on (see there).  On a MPAS_DYC_HOST_ONLY
 * context the flags are kept (mpas_dyc_plan_exchanges plans the step they describe, and the exclusions
 * above hold) and nothing else happens. */
#define MPAS_DYC_PHYSICS_MICROPHYSICS 4
int mpas_dyc_set_physics(mpas_dyc_ctx* ctx, int32_t flags);
/* Incremental analysis update: the branch of atm_srk3 after physics_get_tend
 * (mpas_atm_time_integration.F:459-469 -> atm_add_tend_anal_incr, mpas_atm_iau.F:81-217).  The host sets
 * the analysis-minus-background increments of the reference's tend_iau pool (Registry.xml:3101-3132,
 * the `iau` input stream) with mpas_dyc_set_field(ctx, "tend_iau", name, ...):
 *   tend_iau.u (K, nEdges+1), tend_iau.theta and tend_iau.rho (K, nCells+1),
 *   tend_iau.scalars (ns, K, nCells+1; scalar-major in HBM like state.scalars);
 * the pool is allocated at its first set_field or at mpas_dyc_set_iau(on), and is zero until set.  With
 * IAU on, every mpas_dyc_timestep whose itimestep <= nint(window_length_s / dt) adds, on the owned
 * edges and cells and with wgt = 1 / window_length_s, in the Fortran's operand order,
 *   tend_ru_physics     += wgt rho_edge u_amb                                             (:170)
 *   tend_rho_physics    += wgt rho_amb / zz                                               (:177)
 *   scalars_tend(moist) += wgt (scalars_amb rho_zz + scalars rho_amb / zz)                (:198-199)
 *   tend_rtheta_physics += (1 + Rv/Rd qv) wgt (theta_amb rho_zz + theta rho_amb / zz)
 *                          + Rv/Rd theta scalars_tend(qv),   theta = theta_m / (1 + Rv/Rd qv)  (:190-209)
 * from rho_edge of the previous solve_diagnostics and theta_m, rho_zz, scalars of time level 1; no w
 * forcing (:145).  The sums go into arrays of the library's own, which the step reads in place of
 * tend_physics.*: what the host set there stays as it set it (the reference refills its module scratch
 * every step; here a host may set the arrays once).  tend.scalars_tend is updated in place, as in the
 * reference: the host sets it before every step when it supplies physics tendencies.
 * IAU on implies the step of MPAS_DYC_PHYSICS_TENDENCIES for as long as it is on, after the window
 * too -- scalars_tend feeds the scalar transport instead of being zeroed there (3437, 3743), and
 * negative scalars of time level 2 are set to zero at the end of the step (1645-1646) -- because the
 * reference without DO_PHYSICS would drop the moisture increments.  A host that has not set that flag
 * itself gets what it would have supplied: tend_*_physics of 0.0, and a scalars_tend that is 0.0 before
 * the IAU term of every step.  MPAS_DYC_PHYSICS_RQVDYNTEN and _MICROPHYSICS are not implied.
 * on = config_IAU_option ('off' = 0, 'on' = 1); window_length_s = config_IAU_window_length_s
 * (Registry.xml:355-362), <= 0 with on = 1: MPAS_DYC_EINVAL.  A captured step (mpas_dyc_use_graph) is
 * kept per branch -- forced, with the two IAU kernels, and unforced, without them -- so a run past its
 * window pays nothing and no step is captured again because itimestep changed; changing the switch
 * or the window drops the captured steps.  Works on MPAS_DYC_HOST_ONLY contexts (for
 * mpas_dyc_iau_weight; the field calls there return MPAS_DYC_ESTATE as always). */
int mpas_dyc_set_iau(mpas_dyc_ctx* ctx, int32_t on, double window_length_s);
/* atm_iau_coef (mpas_atm_iau.F:22-78) of step itimestep: *wgt = 1 / window_length_s if itimestep <=
 * nint(window_length_s / dt) (halves round away from zero), else 0; 0 with IAU off.  A weight <= 1e-12
 * leaves the step unforced (:118).  Works on MPAS_DYC_HOST_ONLY contexts. */
int mpas_dyc_iau_weight(const mpas_dyc_ctx* ctx, double dt, int32_t itimestep, double* wgt);
/* The end of atm_srk3 after the host's microphysics (see MPAS_DYC_PHYSICS_MICROPHYSICS); call it
 * before mpas_dyc_shift_time_levels.  Asynchronous. */
int mpas_dyc_finish_step(mpas_dyc_ctx* ctx, double dt);
/* The convective running maxima between history writes: mpas_atm_diag_update (mpas_atm_core.F:700) ->
 * convective_diagnostics_update (diagnostics/convective_diagnostics.F:99-198), on the device, so a run
 * that writes them need not copy the state to the host after every step.  The fields are
 *   diag.w_velocity_max, diag.wind_speed_level1_max, diag.updraft_helicity_max, each (nCells+1);
 * they are allocated, zeroed, at the first mpas_dyc_set_field of one of them or at
 * mpas_dyc_set_diag_update with a non-zero mask -- a context that asks for neither holds none of them
 * and behaves as before -- and mpas_dyc_set_field / get_field / field_bytes / field_device_ptr work on
 * them from then on (a restart puts them back with set_field).
 * mpas_dyc_set_diag_update(flags): which maxima mpas_dyc_diag_update advances, the reference's
 * is_needed_* switches (:33-35, :71-83). Unknown bits: MPAS_DYC_EINVAL.  On a MPAS_DYC_HOST_ONLY context the
 * mask is kept and nothing is allocated. */
#define MPAS_DYC_DIAG_W_VELOCITY_MAX 1           /* is_needed_w_max */
#define MPAS_DYC_DIAG_WIND_SPEED_LEVEL1_MAX 2    /* is_needed_lml_wsp_max */
#define MPAS_DYC_DIAG_UPDRAFT_HELICITY_MAX 4     /* is_needed_updraft_helicity */
int mpas_dyc_set_diag_update(mpas_dyc_ctx* ctx, int32_t flags);
/* convective_diagnostics_update of every block, on the cells 1..nCellsSolve (halo cells and the garbage
 * slot keep what they hold), from w of time level 1 -- call it after mpas_dyc_shift_time_levels, the
 * order of mpas_atm_core.F:664-700 -- and from diag.vorticity and diag.uReconstructZonal / Meridional
 * as the last step (or mpas_dyc_init_diagnostics) left them:
 *   w_velocity_max        = max(old, maxval(w(1:K)))                 interface K+1 is not part of it (:156)
 *   wind_speed_level1_max = max(old, sqrt(uz(1)**2 + um(1)**2))                                    (:162)
 *   updraft_helicity_max  = max(old, uph),
 *     uph   = sum_k uh(k) max(0, min(z(k+1), 5000) - max(z(k), 2000)),  z(k) = zgrid(k) - zgrid(1),
 *             added in ascending k from 0.0                                  (integral_zstaggered, :548-565)
 *     uh(k) = max(0, 0.5 (w(k) + w(k+1))) max(0, zeta(k) / areaCell)                           (:177-178)
 *     zeta(k) = sum of kiteAreasOnVertex(j,v) vorticity(k,v) over the (v, j) with cellsOnVertex(j,v) =
 *             the cell, added in ascending block-local v from 0.0, as the reference's scatter over
 *             the vertices adds them (:169-174) -- not in verticesOnCell order.
 * Every operation in the Fortran's order (fp64, no contraction), so the result has the reference's
 * bits for the block's own numbering; a decomposed run's updraft_helicity_max therefore differs from
 * the one-block run's in the last bits exactly as the reference's does, and the other two do not.
 * Levels outside the 2-5 km band contribute an exact zero for finite inputs and are skipped, with
 * their vorticity gathers: an Inf outside the band does not make the sum NaN here.  Results are
 * guaranteed for finite inputs (Fortran's max with a NaN is unspecified).
 * MPAS_DYC_DIAG_UPDRAFT_HELICITY_MAX needs mesh.areaCell (the reference divides by it) and
 * mesh.cellsOnVertex, kiteAreasOnVertex, zgrid: MPAS_DYC_ESTATE if areaCell or cellsOnVertex is not set.
 * The (v, j) table is derived from cellsOnVertex when the mesh is packed and again after every new
 * mpas_dyc_set_field of cellsOnVertex.
 * Asynchronous on the compute stream (synchronous only while mpas_dyc_set_profile is on, which times
 * it: mpas_dyc_get_profile out[6]); one launch per block, always eager, never part of the step's
 * captured graph, which stays as it is.  Mask 0: does nothing.  MPAS_DYC_ESTATE between
 * mpas_dyc_timestep and mpas_dyc_finish_step with MPAS_DYC_PHYSICS_MICROPHYSICS (time level 2 is not
 * final yet) and on MPAS_DYC_HOST_ONLY contexts. */
int mpas_dyc_diag_update(mpas_dyc_ctx* ctx);
/* convective_diagnostics_reset (:501-525), after a history write: the fields named by flags
 * (MPAS_DYC_DIAG_*) are set to 0.0 over the whole array, halo and garbage slot included, whatever the
 * update mask is.  Asynchronous.  Unknown bits: MPAS_DYC_EINVAL; fields never allocated: nothing to
 * do; MPAS_DYC_HOST_ONLY: MPAS_DYC_ESTATE. */
int mpas_dyc_diag_reset(mpas_dyc_ctx* ctx, int32_t flags);
/* The cloud microphysics call of atm_srk3 (mpas_atm_time_integration.F:1650-1660) on the device, for
 * config_microp_scheme = 'mp_kessler': everything driver_microphysics does for that scheme --
 * precip_from_MPAS, microphysics_from_MPAS, kessler (physics_wrf/module_mp_kessler.F, dt_microp = dt,
 * n_microp = 1), precip_to_MPAS, microphysics_to_MPAS (mpas_atmphys_interface.F:473-785,
 * mpas_atmphys_driver_microphysics.F:429-583) -- on the cells 1..nCellsSolve of every block, one kernel
 * launch per block (kessler.hip), fp64 in the Fortran's operand order.  It updates, on the given time
 * level, state.theta_m and the scalars index_qv / index_qc / index_qr, and diag.rtheta_p, exner,
 * pressure_p, tend.rt_diabatic_tend, and the fields
 *   diag_physics.rainnc, rainncv, precipw (fp64) and i_rainnc (int32), diag.surface_pressure,
 *   tend.tend_sfc_pressure, each (nCells+1);
 * these are allocated, zeroed, at the first mpas_dyc_set_field of one of them or when the switch goes on
 * -- a context that asks for neither holds none of them (mpas_dyc_field_bytes returns 0) and behaves as
 * before -- and set_field / get_field / field_bytes / field_device_ptr work on them from then on (a
 * restart puts rainnc, i_rainnc and surface_pressure back with set_field).  Halo cells and the garbage
 * slot keep what they hold: the step's first exchange refreshes theta_m, scalars, rtheta_p, exner and
 * pressure_p there.  Not part of it: the l_diags branch (compute_relhum); Thompson and WSM6 stay with
 * the host (MPAS_DYC_PHYSICS_MICROPHYSICS).
 * mpas_dyc_set_microphysics(scheme, index_qc, index_qr, bucket_rainnc): with MPAS_DYC_MICROP_KESSLER,
 * every mpas_dyc_timestep runs the scheme on time level 2 after the negative-scalar clip (1645-1646)
 * and before the end of the step (the regional reset, summarize_timestep), captured with the step (the
 * sedimentation's data-dependent split loop is inside the kernel).  index_qc / index_qr are the 1-based
 * scalar indices of cloud and rain water (index_qv is the context's); bucket_rainnc =
 * config_bucket_rainnc (> 0: rainnc above it moves one bucket into i_rainnc).  While on it implies the
 * step of MPAS_DYC_PHYSICS_TENDENCIES, as mpas_dyc_set_iau does and for the same reason (the call sits
 * inside the reference's DO_PHYSICS block), and the step reads tend.rt_diabatic_tend.  Changing the
 * switch drops the captured steps.  MPAS_DYC_MICROP_OFF after steps have run clears nothing:
 * tend.rt_diabatic_tend keeps the scheme's last values and the following steps go on reading them, as
 * the reference's do with whatever its microphysics left there -- from then on the field is the host's
 * to manage, as on the MPAS_DYC_PHYSICS_MICROPHYSICS path (a host that takes the microphysics over
 * writes it after every step; one that runs none sets it to zero).  MPAS_DYC_EINVAL: an unknown scheme, an index outside
 * 1..num_scalars, two of index_qv / index_qc / index_qr equal; MPAS_DYC_ESTATE: together with
 * MPAS_DYC_PHYSICS_MICROPHYSICS (the host's microphysics), in whichever order the two are set.  On a
 * MPAS_DYC_HOST_ONLY context the switch is kept and nothing is allocated. */
#define MPAS_DYC_MICROP_OFF 0
#define MPAS_DYC_MICROP_KESSLER 1
int mpas_dyc_set_microphysics(mpas_dyc_ctx* ctx, int32_t scheme, int32_t index_qc, int32_t index_qr,
                              double bucket_rainnc);
/* The same call eager and on its own, for tests and hosts that sequence the step themselves: the
 * scheme set by mpas_dyc_set_microphysics (MPAS_DYC_ESTATE if off, or on a MPAS_DYC_HOST_ONLY context)
 * with dt_microp = dt on time_level (1 or 2).  Asynchronous on the compute stream (synchronous only
 * while mpas_dyc_set_profile is on, which times it: mpas_dyc_get_profile out[7]). */
int mpas_dyc_microphysics(mpas_dyc_ctx* ctx, double dt, int32_t time_level);
/* The coupling of the physics tendencies to the dynamics, physics_get_tend
 * (physics/mpas_atmphys_todynamics.F:59-434, called at mpas_atm_time_integration.F:424-449), on the device
 * (todynamics.hip), so a host with PBL, convection or radiation schemes uploads a raw tendency only when a
 * scheme has produced a new one and never needs the state back for the coupling.  The inputs are the raw
 * tendencies of the tend_physics pool,
 *   rublten rvblten rthblten rqvblten rqcblten rqiblten rniblten rucuten rvcuten rthcuten rqvcuten rqccuten
 *   rqrcuten rqicuten rqscuten rthratenlw rthratensw, each (K, nCells+1),
 * and mesh.east / mesh.north (3, nCells+1; init_dirs_forphys, mpas_atmphys_init.F:427-439) and
 * mesh.edgeNormalVectors (3, nEdges+1), which the host sets.  It keeps tend_physics.rublten_Edge /
 * rucuten_Edge and diag.tend_u_phys, each (K, nEdges+1).  All of these but edgeNormalVectors are allocated,
 * zeroed, at the first mpas_dyc_set_field of one of them or when the switch goes on -- a context that asks
 * for neither holds none of them (mpas_dyc_field_bytes returns 0) -- and set_field / get_field /
 * field_bytes / field_device_ptr work on them from then on.  No buffer rotation of the step touches them:
 * their device pointers are stable for the life of the context, so a scheme or emulator that lives on
 * the GPU may write its tendencies through mpas_dyc_field_device_ptr, on the compute stream or ordered
 * with it.
 * The results go to the arrays a host that couples by itself uploads (MPAS_DYC_PHYSICS_TENDENCIES):
 * tend_physics.tend_ru_physics, tend_rtheta_physics, tend_rho_physics (= 0) and tend.scalars_tend, with the
 * reference's bits (fp64, the Fortran's operand order, no contraction): tend_toEdges (:494-510) on every
 * edge of the block, each dot product as (n1 e1 + n2 e2) + n3 e3; the mass-weighted sums in the order PBL,
 * convection, longwave, shortwave (:343-422); the theta_m conversion (:426-432).  Elements outside the
 * owned range, the garbage slot included, and every plane of scalars_tend that no scheme touches (:178)
 * are 0.0.  mass is rho_zz of time level 1 (time level 2 has the same bits after
 * atm_rk_integration_setup), theta_m and scalars are time level 1, rho_edge is the last
 * atm_compute_solve_diagnostics'.
 * mpas_dyc_set_todynamics(flags, index_qc, index_qr, index_qi, index_qs, index_ni): non-zero flags make
 * every mpas_dyc_timestep run the coupling after the moist coefficients and before the IAU add, captured
 * with the step, and imply the step of MPAS_DYC_PHYSICS_TENDENCIES as mpas_dyc_set_iau does;
 * MPAS_DYC_TODYN_RQVDYNTEN makes the step compute tend_physics.rqvdynten as MPAS_DYC_PHYSICS_RQVDYNTEN
 * does.  The indices are the 1-based scalar indices (index_qv is the context's).  An index <= 0 means the
 * scalar is absent and its terms are skipped -- the reference would index outside the array there.
 * Reference quirk kept: tend_u_phys is assigned only under the PBL branch (:334), so with the PBL off and a
 * Tiedtke scheme it accumulates rucuten_Edge from call to call (:393-394).
 * On blocks with exchange lists the halos of rublten / rvblten (MPAS_DYC_TODYN_PBL) and rucuten / rvcuten
 * (MPAS_DYC_TODYN_CU_WINDS) are exchanged before the projection (:474-492), as one exchange point of the
 * step, on every transport; without those flags the step's exchange plan is unchanged.
 * MPAS_DYC_EINVAL: unknown bits, a sub-flag without its parent (_PBL_MYNN without _PBL; _CU_KF or
 * _CU_WINDS without _CU), _CU_KF together with _CU_WINDS, an index above num_scalars or equal to
 * index_qv.  MPAS_DYC_ESTATE: together with MPAS_DYC_PHYSICS_TENDENCIES (the host's coupled arrays), in
 * whichever order the two are set.  A step, or mpas_dyc_physics_get_tend, with a wind flag on and
 * mesh.east, mesh.north or mesh.edgeNormalVectors never set: MPAS_DYC_ESTATE naming the input.  Changing
 * the setting drops the captured steps; uploading a raw tendency does not.  flags = 0: off, and the four
 * coupled arrays are set to 0.0 (a step that keeps the physics form, for IAU or the device microphysics,
 * then reads zeros, not the last coupling's values; a host that takes the coupling over uploads its own);
 * a context that never calls it behaves as before.  On a MPAS_DYC_HOST_ONLY context the setting is kept (for
 * mpas_dyc_plan_exchanges) and nothing is allocated. */
#define MPAS_DYC_TODYN_PBL 1          /* config_pbl_scheme /= 'off' */
#define MPAS_DYC_TODYN_PBL_MYNN 2     /* bl_mynn: rniblten */
#define MPAS_DYC_TODYN_CU 4           /* config_convection_scheme /= 'off' */
#define MPAS_DYC_TODYN_CU_KF 8        /* cu_kain_fritsch: rqrcuten, rqscuten */
#define MPAS_DYC_TODYN_CU_WINDS 16    /* cu_tiedtke / cu_ntiedtke: rucuten, rvcuten */
#define MPAS_DYC_TODYN_LW 32          /* config_radt_lw_scheme /= 'off' */
#define MPAS_DYC_TODYN_SW 64          /* config_radt_sw_scheme /= 'off' */
#define MPAS_DYC_TODYN_RQVDYNTEN 128  /* the step also computes rqvdynten (1629-1643) */
int mpas_dyc_set_todynamics(mpas_dyc_ctx* ctx, int32_t flags, int32_t index_qc, int32_t index_qr,
                            int32_t index_qi, int32_t index_qs, int32_t index_ni);
/* The coupling once, eager and on its own, on time level 1: for hosts that want the coupled arrays, and
 * for tests.  MPAS_DYC_ESTATE if off, between mpas_dyc_timestep and mpas_dyc_finish_step, or on a
 * MPAS_DYC_HOST_ONLY context.  Asynchronous on the compute stream (synchronous only while
 * mpas_dyc_set_profile is on, which times it: mpas_dyc_get_profile out[12]).  Collective across ranks
 * when a wind flag is on (the halo exchange). */
int mpas_dyc_physics_get_tend(mpas_dyc_ctx* ctx);
/* The isobaric output diagnostics and mslp of the reference's `diagnostics` stream
 * (diagnostics/isobaric_diagnostics.F, Registry_isobaric.xml), on the device (isobaric.hip), so a run
 * that writes them need not copy ten 3-D fields to the host at output time.  One bit per group, because
 * the reference computes a whole group when any member of it will be written (:96-259).  The fields are
 * in the diag pool, Fortran images with the garbage slot:
 *   <group>_{200,250,500,700,850,925}hPa for the first eight groups, each (nCells+1), vorticity_*hPa
 *   (nVertices+1); mslp, meanT_500_300 (nCells+1); t_isobaric (5, nCells+1), z_isobaric (13, nCells+1);
 *   t_iso_levels (5), z_iso_levels (13); and the one new input relhum (nVertLevels, nCells+1).
 * They are allocated, zeroed, at the first mpas_dyc_set_field of one of them or at mpas_dyc_set_isobaric
 * with a non-zero mask -- a context that asks for neither holds none of them (mpas_dyc_field_bytes
 * returns 0) and behaves as before -- and set_field / get_field / field_bytes / field_device_ptr work
 * on them from then on.  t_iso_levels (30000 .. 50000 Pa) and z_iso_levels (30000 .. 90000 Pa) are filled
 * with the reference's constants (:479-501) when the group is allocated.  diag.relhum is an input: the
 * reference's compute_relhum belongs to the physics' l_diags branch and stays with the host, which sets
 * the field; it is 0.0 until set.
 * mpas_dyc_set_isobaric(flags): the groups mpas_dyc_isobaric_diagnostics computes.  Unknown bits:
 * MPAS_DYC_EINVAL.  On a MPAS_DYC_HOST_ONLY context the mask is kept and nothing is allocated. */
#define MPAS_DYC_ISO_TEMPERATURE   1     /* temperature_{200,250,500,700,850,925}hPa      NEED_TEMP        */
#define MPAS_DYC_ISO_RELHUM        2     /* relhum_*hPa                                   NEED_RELHUM      */
#define MPAS_DYC_ISO_DEWPOINT      4     /* dewpoint_*hPa                                 NEED_DEWPOINT    */
#define MPAS_DYC_ISO_UZONAL        8     /* uzonal_*hPa                                   NEED_UZONAL      */
#define MPAS_DYC_ISO_UMERIDIONAL   16    /* umeridional_*hPa                              NEED_UMERIDIONAL */
#define MPAS_DYC_ISO_HEIGHT        32    /* height_*hPa                                   NEED_HEIGHT      */
#define MPAS_DYC_ISO_W             64    /* w_*hPa                                        NEED_W           */
#define MPAS_DYC_ISO_VORTICITY     128   /* vorticity_*hPa (per vertex)                   NEED_VORTICITY   */
#define MPAS_DYC_ISO_MSLP          256   /* mslp                                          need_mslp        */
#define MPAS_DYC_ISO_T_ISOBARIC    512   /* t_isobaric (5, nCells+1), t_iso_levels        need_t_isobaric  */
#define MPAS_DYC_ISO_Z_ISOBARIC    1024  /* z_isobaric (13, nCells+1), z_iso_levels       need_z_isobaric  */
#define MPAS_DYC_ISO_MEANT_500_300 2048  /* meanT_500_300                                 need_meanT_500_300 */
int mpas_dyc_set_isobaric(mpas_dyc_ctx* ctx, int32_t flags);
/* interp_diagnostics(mesh, state, time_level, diag) (:265-895) of every block with the mask of
 * mpas_dyc_set_isobaric, on the cells 1..nCellsSolve and the vertices 1..nVerticesSolve (halo elements
 * and the garbage slot keep what they hold; the reference loops to nCells / nVertices, but its streams
 * write owned elements only).  It reads w, theta_m and scalars(index_qv) of time_level (1 or 2; the
 * reference passes 1, after the shift), diag.exner, pressure_p, pressure_base, relhum, and
 * diag.vorticity and uReconstructZonal / Meridional as the last step left them, and mesh.zgrid;
 * MPAS_DYC_ISO_VORTICITY also mesh.cellsOnVertex (the garbage cell's slot included), kiteAreasOnVertex
 * and areaTriangle.  fp64 in the Fortran's operand order, no contraction:
 *   pressure(k) = (pressure_p + pressure_base) / 100 (hPa); pressure2 at the K+1 interfaces (:517-542,
 *   the top one through exp / log); pressure_v (:545-555); temperature and the Bolton dewpoint
 *   (:561-569); interp_tofixed_pressure (:899-985) to 200 .. 925 hPa; t_isobaric / z_isobaric on
 *   100 pressure / 100 pressure2 against levels in Pa; compute_layer_mean (:1139-1245);
 *   mslp = 100 compute_slp (:988-1121).
 * interp_tofixed_pressure couples the columns of a block only where some column's pressure is not
 * strictly monotone; results are guaranteed for strictly monotone columns only, where the routine is
 *   p(k+1) < p_out <= p(k) for some k:  (f(k+1) dpl + f(k) dpu) / (dpl + dpu), dpu = p_out - p(k+1),
 *                                       dpl = p(k) - p_out;
 *   else p_out < p(top): f(top) p_out / p(top);  else p_out > p(bottom): f(bottom);
 *   else (p_out == p(top)): the bracket formula on the two topmost levels.
 * compute_slp's failure paths (no level 100 hPa above the ground; klo == khi) set the whole block's
 * mslp to 0.0, without a host synchronisation; the failure test runs over the owned cells only, not
 * over 1..nCells as in the reference.
 * Everything that does not pass through log / exp / pow has the reference's bits; dewpoint_*, mslp and
 * whatever is interpolated in a bracket that contains the top interface's pressure2(K+1) pass through
 * the device library's functions and agree with the C library's to the last bits.
 * With MPAS_DYC_ISO_VORTICITY on a context that has exchange lists the call first exchanges the halo of
 * diag.pressure_p, as mpas_dyc_halo_exchange(ctx, "diag", "pressure_p", 1, 7) does (:397-398): the vertex
 * pressure of an owned vertex reads halo cells.  The call is therefore COLLECTIVE across ranks, like
 * mpas_dyc_halo_exchange: every rank calls it, with the same mask.  No other bit needs a halo.
 * Asynchronous on the compute stream (synchronous only while mpas_dyc_set_profile is on, which times
 * its kernels: mpas_dyc_get_profile out[8]); always eager, never part of the step's captured graph,
 * which stays as it is.  Mask 0: does nothing.  MPAS_DYC_EINVAL: time_level other than 1 or 2.
 * MPAS_DYC_ESTATE: a MPAS_DYC_HOST_ONLY context; MPAS_DYC_ISO_VORTICITY without mesh.areaTriangle,
 * kiteAreasOnVertex or cellsOnVertex set; between mpas_dyc_timestep and mpas_dyc_finish_step with
 * MPAS_DYC_PHYSICS_MICROPHYSICS. */
int mpas_dyc_isobaric_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level);
/* The Ertel PV and dynamic-tropopause diagnostics of the reference's PV stream
 * (diagnostics/pv_diagnostics.F, Registry_pv.xml), on the device (pv.hip), so a run that writes them need
 * not copy w, theta_m, rho_zz, qv, uReconstructX/Y/Z and vorticity to the host at output time.  The
 * fields, Fortran images with the garbage slot:
 *   outputs, diag pool: ertel_pv (nVertLevels, nCells+1) in PVU; iLev_DT (int32, nCells+1), the level
 *     above the dynamic tropopause (0: the whole column is above 2 PVU, nVertLevels+1: below); u_pv, v_pv,
 *     theta_pv, vort_pv (nCells+1), the zonal and meridional wind, theta and the cell's vertical vorticity
 *     on the 2-PVU surface;
 *   inputs the host sets, mesh pool, as mpas_initialize_vectors leaves them: cellTangentPlane
 *     (3, 2, nCells+1), localVerticalUnitVectors (3, nCells+1), edgeNormalVectors (3, nEdges+1).
 * They are allocated, zeroed, at the first mpas_dyc_set_field of one of them or at mpas_dyc_set_pv(on) --
 * a context that asks for neither holds none of them (mpas_dyc_field_bytes returns 0) and behaves as
 * before.  diag.theta and diag.rho exist already; the call rewrites them on the cells 1..nCells.
 * mpas_dyc_set_pv(on): the switch of mpas_dyc_pv_diagnostics.  On a MPAS_DYC_HOST_ONLY context it is kept
 * and nothing is allocated. */
int mpas_dyc_set_pv(mpas_dyc_ctx* ctx, int32_t on);
/* atm_compute_pv_diagnostics(state, time_level, diag, mesh) (:1218-1289) of every block:
 *   1. theta = theta_m / (1 + rvord qv), rho = rho_zz zz on all cells of the block (:1253-1258);
 *   2. on a context that has exchange lists, the halos of diag.theta, uReconstructX/Y/Z and of w of
 *      time_level (:1270-1274), as mpas_dyc_halo_exchange does: the call is COLLECTIVE across ranks;
 *   3. ertel_pv on the owned cells (calc_epv, :1139-1216): the finite-volume gradients of w and theta over
 *      the cell's edges, centred vertical differences (one-sided at the column's ends), the cell's
 *      vertical vorticity as the kite-area average of diag.vorticity, the Earth's vorticity, divided by
 *      rho, dotted with grad theta, times 1e6;
 *   4. the halo of ertel_pv (:1279-1280);
 *   5. floodFill_tropo (:581-716) over all cells of the block: the cell-levels with ertel_pv sign(lat) < 2
 *      connected to levels 1..min(nVertLevels, 3) through vertical and same-level horizontal neighbours.
 *      That set is the fixed point of the reference's sweeps whatever their order.  A neighbour outside
 *      the block is never in the troposphere, and there is no communication inside the fill: the
 *      reference's behaviour (its :696), so a block's halo columns may differ from their owners';
 *   6. iLev_DT on the cells 1..nCells; 7. interp_pv (:826-899) of the four fields on the owned cells.
 * Halo cells and garbage slots of the four 2-D fields, and iLev_DT's garbage slot, keep what they hold.
 * It reads w, theta_m, rho_zz and scalars(index_qv) of time_level (1 or 2; the reference passes 1), and
 * diag.vorticity and uReconstructX/Y/Z/Zonal/Meridional as the last step left them; mesh.zgrid, zz, latCell,
 * dvEdge, areaCell, kiteAreasOnVertex, the connectivity and the three vector arrays.  fp64 in the Fortran's
 * operand order, no contraction: every output has the reference's bits, with one defined deviation -- at
 * level nVertLevels the reference forms dv_dz from velCellp, a local it never set there (:997), so its
 * ertel_pv(nVertLevels, :) is undefined; this library takes velCellm, as the u line two above it does.
 * The PV budget (calc_pvBudget, depv_dt_*) is mpas_dyc_pv_budget_diagnostics below; floodFill_strato, which
 * the reference never calls, is not provided.
 * SYNCHRONOUS: the fill's sweeps run in small batches and the host reads a flag back after each, so the
 * call returns with the outputs complete.  Always eager, never part of the step's captured graph, which
 * stays as it is.  Under mpas_dyc_set_profile its milliseconds are mpas_dyc_get_profile out[9].
 * Switch off (mpas_dyc_set_pv(0), or never set): does nothing.  MPAS_DYC_EINVAL: time_level other than 1
 * or 2.  MPAS_DYC_ESTATE: a MPAS_DYC_HOST_ONLY context; between mpas_dyc_timestep and
 * mpas_dyc_finish_step with MPAS_DYC_PHYSICS_MICROPHYSICS; a needed mesh input never set (the three vector
 * arrays, areaCell, kiteAreasOnVertex, cellsOnVertex), with a message that names it. */
int mpas_dyc_pv_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level);
/* The Ertel PV budget of the same stream (atm_compute_pvBudget_diagnostics, pv_diagnostics.F:1291-1613), on
 * the device (pvbudget.hip), so a run that writes a depv_dt_* field need not copy the raw theta tendencies,
 * tend_u_phys, tend.u_euler / w_euler / theta_euler, rho_edge and the PV diagnostics' inputs to the host at
 * output time.  The mask: */
#define MPAS_DYC_PVB_ON 1    /* any depv_dt_* / dtheta_dt_mp will be written */
#define MPAS_DYC_PVB_LW 2    /* rthratenlw is associated */
#define MPAS_DYC_PVB_SW 4    /* rthratensw */
#define MPAS_DYC_PVB_BL 8    /* rthblten  */
#define MPAS_DYC_PVB_CU 16   /* rthcuten  */
/* The fields, Fortran images with the garbage slot, diag pool: depv_dt_lw, depv_dt_sw, depv_dt_bl, depv_dt_cu,
 * depv_dt_mp, depv_dt_mix, depv_dt_diab, depv_dt_fric (nVertLevels, nCells+1) in PVU/s; dtheta_dt_mp (an
 * input: the host's microphysics heating, 0.0 until set) and dtheta_dt_mix (written by the call on the cells
 * 1..nCells), the same shape; depv_dt_diab_pv, depv_dt_fric_pv (nCells+1), the two on the 2-PVU surface.  With
 * the library's scratch arrays they are allocated, zeroed, at the first mpas_dyc_set_field of one of them or
 * at mpas_dyc_set_pv_budget with MPAS_DYC_PVB_ON -- a context that asks for neither holds none of them.
 * mpas_dyc_set_pv_budget(flags): 0 switches the budget off and is always allowed.  A source bit says that the
 * raw tendency of tend_physics is associated (its scheme runs); a source whose bit is off contributes exact
 * zeros and is not read.  MPAS_DYC_EINVAL: unknown bits; a source bit without MPAS_DYC_PVB_ON.
 * MPAS_DYC_ESTATE: MPAS_DYC_PVB_ON while mpas_dyc_set_pv is off.  On a MPAS_DYC_HOST_ONLY context the mask is
 * kept and nothing is allocated. */
int mpas_dyc_set_pv_budget(mpas_dyc_ctx* ctx, int32_t flags);
/* The reference's pv_diagnostics_compute when a budget field is written: mpas_dyc_pv_diagnostics (unchanged)
 * and then, on the same time level,
 *   1. on a context that has exchange lists, the halos the reference exchanges (:1592-1605): the raw theta
 *      tendencies whose bits are set, dtheta_dt_mp, tend_u_phys, tend.u_euler and tend.w_euler (COLLECTIVE);
 *   2. dtheta_dt_mix = tend.theta_euler / (1 + rvord qv) on all cells (:1578-1584), then its halo;
 *   3. F = tend_u_phys + tend.u_euler / rho_edge on all edges (:1477-1481; without diag.tend_u_phys, which
 *      only mpas_dyc_set_todynamics allocates, the literal 0.0 takes its place) and tend.w_euler over the
 *      density at the interfaces on all cells (:1492-1501);
 *   4. calc_vertical_curl of F on all vertices (:1113-1137): a vertex sums its valid edges in ascending
 *      local edge index, as the reference's edge loop reaches them; mpas_reconstruct of F on the owned cells;
 *   5. on the owned cells depv_dt_{lw,sw,bl,cu,mp,mix} = ((curl u + 2 Omega) / rho) . grad(source) 1e6 and
 *      their sum depv_dt_diab = ((((lw + sw) + bl) + cu) + mp) + mix (:1386-1473; mix is guarded by
 *      dtheta_dt_mp's association as in the reference, :1460, which always holds here), and depv_dt_fric =
 *      curl(F, uncoupled tend_w) . (grad theta / rho) 1e6 (:1503-1529);
 *   6. depv_dt_diab_pv and depv_dt_fric_pv: interp_pv with the iLev_DT and ertel_pv just computed (:786-824).
 *      The fill gives iLev_DT = 0 or >= 2, never 1; for 1 the reference's interp_pv would read level 0, the
 *      element before the column in memory.  Should a column hold 1 all the same, this library reads level 1
 *      in its place (the lower level clamped into the column): defined differently from the reference
 *      (and from the numpy restatement, which repeats the reference's read) there.
 * fp64 in the Fortran's operand order, no contraction: the reference's bits below level nVertLevels (there
 * mpas_dyc_pv_diagnostics' deviation carries over: dv_dz takes velCellm), with two more defined deviations.
 * The reference overwrites tend_u_phys and tend.w_euler in place (:1479, :1496-1501); this library leaves
 * both untouched and works in scratch, so a second call gives the same bits and the next step's
 * physics_get_tend accumulation is not polluted.  And the outputs are written on the owned cells only: the
 * reference's whole-array depv_dt_diab sum also covers halo columns that nothing computed.
 * It reads what mpas_dyc_pv_diagnostics reads, the tendencies named above, diag.rho_edge, mesh.dcEdge,
 * areaTriangle, verticesOnEdge, edgesOnVertex and coeffs_reconstruct.  SYNCHRONOUS like
 * mpas_dyc_pv_diagnostics; always eager, never part of the step's captured graph.  Under
 * mpas_dyc_set_profile its milliseconds, the PV diagnostics included, are mpas_dyc_get_profile out[13].
 * Switch off: does nothing and allocates nothing.  Errors: those of mpas_dyc_pv_diagnostics, and
 * MPAS_DYC_ESTATE when mpas_dyc_set_pv is off; when mesh.coeffs_reconstruct was neither computed
 * (mpas_dyc_init_reconstruct) nor set, or mesh.areaTriangle never set; when a source bit is set but its raw
 * array was never allocated -- each with a message that names the field. */
int mpas_dyc_pv_budget_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level);
/* The output-time half of the reference's convective diagnostics (diagnostics/convective_diagnostics.F,
 * Registry_convective.xml), on the device (convcompute.hip): convective_diagnostics_compute (:227-487) with
 * getcape (:595-1037), so a run that writes cape, cin or the helicities need not copy theta_m, qv, exner,
 * pressure_p, pressure_base and the reconstructed winds to the host and lift every column there.  One bit
 * per output, in the order of the reference's list (:285-312); the diag fields have the reference's
 * names, lower case (cape, cin, lcl, lfc, srh_0_1km, srh_0_3km, uzonal_surface, uzonal_1km, uzonal_6km,
 * umeridional_surface, umeridional_1km, umeridional_6km, temperature_surface, dewpoint_surface), each
 * (nCells + 1). */
#define MPAS_DYC_CONV_CAPE 1
#define MPAS_DYC_CONV_CIN 2
#define MPAS_DYC_CONV_LCL 4
#define MPAS_DYC_CONV_LFC 8
#define MPAS_DYC_CONV_SRH_0_1KM 16
#define MPAS_DYC_CONV_SRH_0_3KM 32
#define MPAS_DYC_CONV_UZONAL_SURFACE 64
#define MPAS_DYC_CONV_UZONAL_1KM 128
#define MPAS_DYC_CONV_UZONAL_6KM 256
#define MPAS_DYC_CONV_UMERIDIONAL_SURFACE 512
#define MPAS_DYC_CONV_UMERIDIONAL_1KM 1024
#define MPAS_DYC_CONV_UMERIDIONAL_6KM 2048
#define MPAS_DYC_CONV_TEMPERATURE_SURFACE 4096
#define MPAS_DYC_CONV_DEWPOINT_SURFACE 8192
#define MPAS_DYC_CONV_ALL 16383
/* mpas_dyc_set_convective(flags): the mask mpas_dyc_convective_diagnostics applies.  Unknown bits:
 * MPAS_DYC_EINVAL, nothing allocated.  A non-zero mask allocates the fourteen fields, zeroed; so does a
 * first mpas_dyc_set_field of one of them.  A context that asks for neither holds none of them
 * (mpas_dyc_field_bytes returns 0) and behaves as before.  On a MPAS_DYC_HOST_ONLY context the mask is
 * kept and nothing is allocated. */
int mpas_dyc_set_convective(mpas_dyc_ctx* ctx, int32_t flags);
/* convective_diagnostics_compute on the cells 1..nCellsSolve of every block; halo cells and the garbage
 * slot keep what they hold.  The reference's quirks are kept:
 *   - with any bit set, uzonal_surface, umeridional_surface, temperature_surface and dewpoint_surface are
 *     written (level 1 of the winds, of theta_m / (1 + rvord qv) * exner, and of Bolton's dewpoint);
 *   - uzonal / umeridional _1km / _6km (column_height_value at 1000 m and 6000 m above the lowest
 *     interface) and srh_0_1km / srh_0_3km (storm-relative helicity against Bunkers' right-mover motion,
 *     negative contributions discounted) are each written only under their own bit;
 *   - cape and cin (getcape: the most unstable parcel below 500 hPa, pseudoadiabatic, liquid only,
 *     100 Pa sub-steps) are both written if either bit is set;
 *   - lcl and lfc are never written: the reference fetches them and never computes them.  Their bits
 *     only count towards "any".
 * It reads theta_m and scalars(index_qv) of time_level (1 or 2; the reference passes 1), diag.exner,
 * pressure_p, pressure_base, uReconstructZonal / Meridional and mesh.zgrid; not diag.relhum, which the
 * reference fetches and does not use.  fp64 in the Fortran's operand order, no contraction: the nine
 * outputs that are + - * / and sqrt have the reference's bits; cape, cin and dewpoint_surface pass through
 * the device library's exp / log / pow and are within the project's parity bound of them (rel Linf 1e-10)
 * on columns whose branch decisions a 4 ulp drift of those functions does not move.
 * One defined deviation, BOUNDED WORK: a column's ascent ends, with cape and cin as accumulated so far,
 * once it has taken 8192 + nVertLevels sub-steps (a column monotone below 8192 hPa never does; real
 * columns take under a thousand), and int(dp / pinc) counts as at most 2^30; with the reference's own cap
 * of 100 iterations per sub-step (after which it too returns what it has) the call ends whatever the
 * inputs are.
 * Asynchronous on the compute stream, synchronous under mpas_dyc_set_profile (its milliseconds are
 * mpas_dyc_get_profile out[11]).  Always eager, never part of the step's captured graph.  Not collective:
 * no halo is read.  Mask 0: does nothing.  MPAS_DYC_EINVAL: time_level other than 1 or 2.
 * MPAS_DYC_ESTATE: a MPAS_DYC_HOST_ONLY context; between mpas_dyc_timestep and mpas_dyc_finish_step with
 * MPAS_DYC_PHYSICS_MICROPHYSICS.  (A context without scalars does not exist: mpas_dyc_create refuses
 * num_scalars < 1, so there is always a qv, as for mpas_dyc_isobaric_diagnostics.) */
int mpas_dyc_convective_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level);
/* Regional lateral boundary conditions, config_apply_lbcs (mpas_atm_time_integration.F:683-778,
 * 934-987, 1109-1180, 1253-1270, 1491-1560, 1672-1790; the routines at 6088-6671).  apply = 1 turns
 * them on (the pair kernel layout is required).  The host sets, as in the reference's lbc pool
 * (mpas_atm_boundaries.F): lbc.lbc_u / lbc_ru (K, nEdges+1), lbc.lbc_rho_zz / lbc_rtheta_m
 * (K, nCells+1) and lbc.lbc_scalars (ns, K, nCells+1), each with time level 1 = the tendency over
 * the current LBC interval and time level 2 = the interval-end state; the mesh's bdyMaskCell,
 * bdyMaskEdge, nearestRelaxationCell, meshScalingRegionalCell / Edge; and, before every step,
 * seconds_to_interval_end = LBC interval end - the step's start time.  A driving value delta
 * seconds into the step is then state - (seconds_to_interval_end - delta) * tendency, as
 * mpas_atm_get_bdy_state (:337-409) computes it.  All scalars are driven. */
int mpas_dyc_set_lbc(mpas_dyc_ctx* ctx, int32_t apply, double seconds_to_interval_end);
/* The model-init precompute of atm_mpas_init_block (mpas_atm_core.F:311-358, 456-458; the routines at
 * 927-1288), on the device, for every block: invAreaCell, invDvEdge, invDcEdge, invAreaTriangle;
 * atm_compute_signs (edgesOnVertex_sign, edgesOnCell_sign, zb_cell, zb3_cell, kiteForCell);
 * atm_adv_coef_compression (nAdvCellsForEdge, advCellsForEdge, adv_coefs, adv_coefs_3rd);
 * atm_couple_coef_3rd_order (config_coef_3rd_order of the context's config);
 * atm_compute_mesh_scaling (meshScalingDel2 / Del4, meshScalingRegionalCell / Edge,
 * config_h_ScaleWithMesh) and atm_compute_damping_coefs (dss, config_zd, config_xnutr).
 * It reads what the init file holds, set beforehand with mpas_dyc_set_field: the connectivity,
 * dcEdge, dvEdge, zgrid and mesh.deriv_two (15, 2, nEdges+1), mesh.zb / zb3 (nVertLevels+1, 2,
 * nEdges+1), mesh.meshDensity, mesh.areaCell (nCells+1), mesh.areaTriangle (nVertices+1).
 * Every + - * / in the reference's order.  Two values are transcendental: meshDensity**0.25 and the
 * damping layer's sin.  Set them too -- mesh.meshDensity_root4 (nCells+1: meshDensity**0.25),
 * mesh.meshDensityEdge_root4 (nEdges+1: ((meshDensity(c1) + meshDensity(c2)) / 2)**0.25) and
 * mesh.dss_sin (nVertLevels, nCells+1: sin(0.5 pi (z - config_zd) / (zt - config_zd)) where z >
 * config_zd), from the C library as the compiled reference calls it -- and the outputs are the
 * reference's bits.  Unset, they are computed on the device correctly rounded; the reference's C library
 * is 1 ulp away for ~0.1 % of arguments, and meshScaling* then differ by up to 2 ulp there, dss by up to
 * 4.  Cells of more than 10 edges are refused (MPAS_DYC_EINVAL).  Synchronous. */
int mpas_dyc_model_init(mpas_dyc_ctx* ctx, int32_t h_scale_with_mesh, double config_zd, double config_xnutr);
/* deriv_two as core_init_atmosphere computes it (mpas_atm_advection.F:21-394,
 * atm_initialize_advection_rk, polynomial_order = 2, on a sphere), into mesh.deriv_two (15, 2, nEdges+1)
 * of one block (allocated if not yet set), on the device.  The transcendental half comes from the
 * caller, per cell and edgesOnCell slot (nCells x maxEdges at the declared stride, slots beyond
 * nEdgesOnCell ignored): xp / yp, the tangent-plane coordinates of cellsOnCell(i) (132-181: cos / sin
 * of thetat(i) times the arc length), and sin_the / cos_the of edgesOnCell(i)'s normal angle thetae
 * (303-315, 334-335 / 347-348).  The least-squares fit -- amatrix, poly_fit_2 with MIGS / ELGS
 * (215-226, 567-741) -- and the weights 2 cos^2 b(4,j) + 2 cos sin b(5,j) + 2 sin^2 b(6,j) (327-358)
 * run here, one thread per cell, in the Fortran's operand order: bit for bit the reference's deriv_two
 * when the inputs are its values (they are the C library's sin / cos / asin, which no device library
 * reproduces; init_atm.deriv_two_inputs computes them that way).  Uses the block's nEdgesOnCell,
 * edgesOnCell and cellsOnEdge.  Cells with more than 14 edges: MPAS_DYC_EINVAL.  Synchronous. */
int mpas_dyc_init_deriv_two(mpas_dyc_ctx* ctx, int32_t block, const double* xp, const double* yp,
                            const double* sin_the, const double* cos_the);
/* zb / zb3, the z-metric terms of the omega equation, as core_init_atmosphere computes them
 * (mpas_init_atm_cases.F:1045-1093) for config_theta_adv_order 2, 3 or 4, into mesh.zb / mesh.zb3
 * (nVertLevels+1, 2, nEdges+1) of one block (allocated if not yet set), on the device, from the block's
 * mesh.deriv_two, zgrid, dcEdge, dvEdge, areaCell and connectivity.  Edges with no owned cell and
 * level nVertLevels+1 are 0.  Bit for bit the reference's arithmetic.  Synchronous. */
int mpas_dyc_init_zb(mpas_dyc_ctx* ctx, int32_t block, int32_t theta_adv_order);
/* The reconstruction coefficients of every block on the device: mpas_rbf_interp_initialize's vectors
 * (operators/mpas_vector_operations.F:697-769: edge normals, each cell's tangent plane) and
 * mpas_init_reconstruct (operators/mpas_vector_reconstruction.F:112-177: the inverse-multiquadric RBF
 * system of each cell's edges with a constant vector in the plane, solved by elgs + mpas_legs), what
 * mpas_atm_core.F:408-409 runs at model init, into mesh.coeffs_reconstruct.  Reads mesh.xCell, yCell,
 * zCell (nCells+1), xEdge, yEdge, zEdge (nEdges+1), set beforehand, and the connectivity.  + - * / sqrt
 * only, in the Fortran's order: bit for bit the reference's coefficients.  Cells with more than 14
 * edges: MPAS_DYC_EINVAL.  Synchronous. */
int mpas_dyc_init_reconstruct(mpas_dyc_ctx* ctx);
/* atm_compute_output_diagnostics(state, time_level, diag, mesh) (mpas_atm_core.F:753, called
 * before history writes at :544 and :694): diag theta, rho and pressure from theta_m, rho_zz,
 * scalars(index_qv) of the time level, zz, pressure_base and pressure_p.  Asynchronous. */
int mpas_dyc_output_diagnostics(mpas_dyc_ctx* ctx, int32_t time_level);

/* ---- summarize_timestep (mpas_atm_time_integration.F:6675-7018, called at the end of atm_srk3, 1794) ----
 * The modes are the namelist switches of the reference; each step reduces the enabled ones on
 * the device (part of mpas_dyc_timestep, captured with the step), and mpas_dyc_get_summary
 * folds the blocks of this process and, over RCCL, all ranks. */
#define MPAS_DYC_PRINT_GLOBAL_MINMAX_VEL 1   /* config_print_global_minmax_vel (default .true.), 6945-6983 */
#define MPAS_DYC_PRINT_DETAILED_MINMAX_VEL 2 /* config_print_detailed_minmax_vel, 6721-6943 */
#define MPAS_DYC_PRINT_GLOBAL_MINMAX_SCA 4   /* config_print_global_minmax_sca, 6986-7016 */

/* One located extreme of the detailed mode: the value, the level and the lat/lon in degrees of
 * the first owned element (cell-major, level-minor) holding it, as the reference's loops find it,
 * reduced over ranks as mpas_dmpar_min/maxattributes_real does (MPI_MINLOC / MPI_MAXLOC per
 * attribute, mpas_dmpar.F:1090-1160).  lon is shifted to (-180, 180] as at 6771-6773. */
typedef struct {
  double value, lat, lon;
  int32_t k;      /* 1-based level (kMax_global); -1 if no element */
  int32_t index;  /* 1-based local index on its block (indexMax); -1 if no element */
} mpas_dyc_extreme;

typedef struct {
  int32_t flags;                     /* the modes the values below were reduced for */
  double w_min, w_max, u_min, u_max; /* global_minmax_vel: min/max over owned w, u starting from 0.0 */
  mpas_dyc_extreme w_min_at, w_max_at, u_min_at, u_max_at, wsp_max_at; /* detailed_minmax_vel */
  int64_t nan_w, nan_u;              /* NaNs in the owned w, u (the detailed mode aborts on any, 6926-6940) */
} mpas_dyc_summary;

/* Modes reduced by every following step (default MPAS_DYC_PRINT_GLOBAL_MINMAX_VEL; 0 = none). */
int mpas_dyc_set_summary(mpas_dyc_ctx* ctx, int32_t flags);
/* The last step's summary over all blocks and ranks (collective when ranks share a communicator:
 * every rank calls it after the same step).  Waits for the step.  scalar_minmax (may be NULL)
 * receives num_scalars (min, max) pairs of the global_minmax_sca mode; n = its length in doubles. */
int mpas_dyc_get_summary(mpas_dyc_ctx* ctx, mpas_dyc_summary* out, double* scalar_minmax, int32_t n);
/* The same for one block of this process, reduced over ranks: the reference writes one set of log
 * lines per block of a task, each reduced over tasks (6945-6983, 6991-7015).  Collective like
 * mpas_dyc_get_summary: every rank calls it for the same block index after the same step. */
int mpas_dyc_get_block_summary(mpas_dyc_ctx* ctx, int32_t block, mpas_dyc_summary* out, double* scalar_minmax,
                               int32_t n);

/* ---- domain decomposition: several blocks per process, halo exchange ----
 *
 * A context holds the blocks this process owns (MPAS domain%blocklist; one per
 * GPU in production, several per GPU in tests).  Each block has its own dims
 * (owned-first element order, nCellsSolve etc. = owned counts, as built by
 * mpas_block_creator.F) and its own fields, addressed with the *_block_field
 * variants (the functions above act on block 0).  Halo exchanges happen inside
 * mpas_dyc_timestep at the reference's mpas_dmpar_exch_halo_field points
 * (mpas_atm_time_integration.F:329-1717, 3757, 4098): block-to-block copies
 * inside the process, RCCL ncclSend/ncclRecv between processes. */
#define MPAS_DYC_CELL 0
#define MPAS_DYC_EDGE 1
#define MPAS_DYC_VERTEX 2
#define MPAS_DYC_SEND 0
#define MPAS_DYC_RECV 1

int mpas_dyc_create_blocks(int32_t nblocks, const mpas_dyc_dims* dims /* [nblocks] */, const mpas_dyc_config* cfg,
                           int device, mpas_dyc_ctx** out);
int32_t mpas_dyc_num_blocks(const mpas_dyc_ctx* ctx);
int mpas_dyc_set_block_field(mpas_dyc_ctx* ctx, int32_t block, const char* pool, const char* name,
                             int32_t time_level, const void* host, int64_t nbytes);
int mpas_dyc_get_block_field(mpas_dyc_ctx* ctx, int32_t block, const char* pool, const char* name,
                             int32_t time_level, void* host, int64_t nbytes);
int64_t mpas_dyc_block_field_bytes(const mpas_dyc_ctx* ctx, int32_t block, const char* pool, const char* name);
void* mpas_dyc_block_field_device_ptr(mpas_dyc_ctx* ctx, int32_t block, const char* pool, const char* name,
                                      int32_t time_level);
/* One entry of a block's multihalo exchange list (mpas_dmpar.F mpas_multihalo_exchange_list:
 * procID/blockID/nList/srcList|destList): the elements of `location` in halo layer
 * `halo_layer` (cells 1..2, edges/vertices 1..3) that this block sends to (owned elements)
 * or receives from (halo elements) block `peer_block` of rank `peer_rank`, as 1-based local
 * indices in message order.  Both sides must list the same elements in the same order. */
int mpas_dyc_set_exchange_list(mpas_dyc_ctx* ctx, int32_t block, int32_t location, int32_t halo_layer,
                               int32_t direction, int32_t peer_rank, int32_t peer_block, const int32_t* local_index,
                               int32_t n);
/* A list of another task as mpas_dmpar keeps it when tasks hold several blocks (parinfo xToSend /
 * xToRecv: endPointID = the task, the other list = buffer positions; mpas_dmpar.F:5448-5535): this
 * block's elements local_index[i] (1-based; owned to send, halo to receive) take 1-based slot
 * position[i] of the (location, halo_layer) region of the one message between this task and task
 * peer_rank, whose slots all blocks of this task fill together.  The message is laid out as
 * mpas_dmpar lays out its buffer -- per field of the exchange, per halo layer a region as long as its
 * largest position -- so a task need not know which block of the peer receives an element.  A peer
 * rank takes either positional lists or block-pair lists (mpas_dyc_set_exchange_list), not both. */
int mpas_dyc_set_exchange_positions(mpas_dyc_ctx* ctx, int32_t block, int32_t location, int32_t halo_layer,
                                    int32_t direction, int32_t peer_rank, const int32_t* local_index,
                                    const int32_t* position, int32_t n);
/* RCCL communicator for exchanges between processes (one rank per GPU): rank 0 creates the
 * id (ncclGetUniqueId), every rank passes it to mpas_dyc_comm_init (ncclCommInitRank).  On failure
 * (MPAS_DYC_ECOMM; e.g. ranks that share a GPU, which RCCL refuses) the context keeps no
 * communicator; with mpas_dyc_comm_init_host on one node the one-sided transfer still carries the
 * halos, without the RCCL fallback. */
int64_t mpas_dyc_comm_unique_id_bytes(void);
int mpas_dyc_comm_unique_id(void* id, int64_t nbytes);
int mpas_dyc_comm_init(mpas_dyc_ctx* ctx, const void* id, int64_t nbytes, int32_t nranks, int32_t rank);
/* Ranks without RCCL: the host's own all-gather (MPI_Allgather, a torch.distributed gloo group, ...)
 * for the few set-up collectives, and the one-sided transfer (mpas_dyc_set_p2p, switched on here) for
 * every halo message -- all ranks on one node.  fn(send, recv, nbytes, user) must place every rank's
 * nbytes in recv in rank order and return 0; it is called from mpas_dyc_timestep /
 * mpas_dyc_init_diagnostics / mpas_dyc_halo_exchange (set-up of new exchange points, on every rank at
 * the same call) and from mpas_dyc_get_summary, never during graph capture.  Instead of
 * mpas_dyc_comm_init, or after it (the Fortran drop-in: MPI_Allgather on dminfo%comm): then the
 * set-up collectives go through fn, and the RCCL communicator stays for the fallback to RCCL groups
 * when the one-sided transfer is unavailable (mpas_dyc_set_p2p).  Also on MPAS_DYC_HOST_ONLY
 * contexts (mpas_dyc_comm_check; the plan dry run). */
typedef int (*mpas_dyc_allgather_fn)(const void* send, void* recv, int64_t nbytes, void* user);
int mpas_dyc_comm_init_host(mpas_dyc_ctx* ctx, int32_t nranks, int32_t rank, mpas_dyc_allgather_fn fn, void* user);
/* Collective check of the context's communicator (the host all-gather of mpas_dyc_comm_init_host, or
 * RCCL's): every rank all-gathers (rank, nranks, node), and the call fails (MPAS_DYC_ECOMM) on every
 * rank if a slot holds another rank or another rank count.  *nodes = the number of distinct nodes
 * the ranks run on (the one-sided transfer needs 1: mpas_dyc_set_p2p).  No counterpart in the
 * reference (mpas_dmpar_init's communicator is taken as given). */
int mpas_dyc_comm_check(mpas_dyc_ctx* ctx, int32_t* nodes);
/* Test hook: route block-to-block exchanges inside this process through RCCL (send to self). */
int mpas_dyc_set_transport(mpas_dyc_ctx* ctx, int32_t rccl_for_local_blocks);
/* One-sided transfer between the ranks of one node (on = 1; 0 = RCCL groups; -1 = the environment
 * variable MPAS_DYCORE_P2P, read at context creation, default 0).  Replaces the ncclSend / ncclRecv
 * groups of every exchange point by kernels that move the halo themselves (halo.hip), with flags in
 * each rank's arena (ready / consumed counters, IPC-mapped by the peers at set-up).  Blocking
 * exchanges with block-pair lists (the default) are pulls: k_p2p_pull copies the peer's owned
 * columns from its fields (IPC-mapped) straight into this rank's halo columns.  Positional lists and
 * split-phase exchanges (MPAS_DYCORE_P2P_PULL=0 for all) keep the send / receive buffers: the pack
 * fills this rank's send buffer (device memory the peers map), k_p2p_post raises ready, and
 * k_p2p_get pulls each peer's message and waits until this rank's own buffer has been pulled.  Same
 * messages and order as the RCCL path (the plans are the ones mpas_dyc_plan_exchanges reports).
 * Set-up runs once per exchange-plan build, over the communicator of mpas_dyc_comm_init (or the host
 * all-gather of mpas_dyc_comm_init_host); if IPC is refused or the ranks span several nodes, every
 * rank drops the transfer together and plans for RCCL (mpas_dyc_get_p2p then returns 0).  A message
 * that does not arrive within 30 s makes mpas_dyc_synchronize return MPAS_DYC_ECOMM.  Collective:
 * every rank calls it with the same value. */
int mpas_dyc_set_p2p(mpas_dyc_ctx* ctx, int32_t on);
/* 1 while the one-sided transfer is on (0 after the set-up found it unavailable on some rank -- IPC
 * refused, ranks on several nodes -- and every rank went back to RCCL, with a line on stderr). */
int mpas_dyc_get_p2p(const mpas_dyc_ctx* ctx);
/* Split-phase exchanges: at the tend_u, rho_pp and rtheta_pp exchanges the interior
 * elements are computed while the halo traffic runs on a second stream.  on = 1 / 0;
 * -1 (default) = automatic: on when exchanges go through RCCL (more than one rank). */
int mpas_dyc_set_overlap(mpas_dyc_ctx* ctx, int32_t on);
/* mpas_dmpar_exch_halo_field(field, haloLayers) for one field; layer_mask bit l-1 = layer l. */
int mpas_dyc_halo_exchange(mpas_dyc_ctx* ctx, const char* pool, const char* name, int32_t time_level,
                           int32_t layer_mask);

/* ---- exchange-plan dry run (no device) ----
 * `device` = MPAS_DYC_HOST_ONLY in mpas_dyc_create(_blocks) makes a context that holds dims,
 * config and exchange lists but no device memory, stream or communicator.  Only
 * mpas_dyc_set_exchange_list, mpas_dyc_set_overlap / _set_transport and
 * mpas_dyc_plan_exchanges work on it (field calls return MPAS_DYC_ESTATE).  It lets a host
 * check, before any GPU is touched, that the RCCL messages every rank will post match: rank r's
 * sends to rank p at an exchange point must be rank p's receives from r there, in the same
 * order and of the same sizes (what ncclGroupStart/End requires, mpas_dmpar.F:5386-5552). */
#define MPAS_DYC_HOST_ONLY (-2)

/* One RCCL message of an exchange point, as the step posts it. */
typedef struct {
  int32_t point;      /* 0-based index of the exchange call in issue order (see below) */
  int32_t direction;  /* MPAS_DYC_SEND (ncclSend) / MPAS_DYC_RECV (ncclRecv) */
  int32_t block;      /* local block that packs / unpacks it */
  int32_t peer_rank, peer_block;
  int64_t count;      /* doubles */
} mpas_dyc_plan_msg;

/* Run the exchange planner as rank `rank` of `nranks` over the calls one model run issues, in
 * order: the model-init exchanges (mpas_dyc_init_diagnostics), then one atm_srk3 on each
 * time-level parity (a step, mpas_dyc_shift_time_levels, a step).  Writes up to `cap` messages
 * (each point's sends, then its receives, in posting order) and sets *n_msgs to the number
 * needed; writes the calls' plan keys, one per line in issue order, into keys[keys_bytes]
 * (NUL-terminated) and sets *keys_len to the bytes needed.  Returns MPAS_DYC_EINVAL when
 * either buffer was too small (the counts are still set). */
int mpas_dyc_plan_exchanges(mpas_dyc_ctx* ctx, int32_t nranks, int32_t rank, double dt, mpas_dyc_plan_msg* msgs,
                            int64_t cap, int64_t* n_msgs, char* keys, int64_t keys_bytes, int64_t* keys_len);

/* 1 if the last mpas_dyc_timestep replayed a captured hipGraph, 0 if it ran eagerly.  With more
 * than one rank a failed capture is an error (MPAS_DYC_EHIP), never a per-rank eager fallback:
 * one eager rank would add ~280 launches per dt to every exchange wait of the others. */
int mpas_dyc_graph_active(const mpas_dyc_ctx* ctx);

/* ---- measurement hooks (bench.py / tests) ---- */
/* A `reps`-sub-step acoustic loop (atm_advance_acoustic_step + atm_divergence_damping_3d per
 * sub-step, srk3 :788-870) of block 0 on the current state, all sub-steps numbered
 * `small_step`, timed with HIP events on the compute stream.  The launches are the ones srk3
 * issues: the edge phase, the cell phase, and for every further sub-step the edge phase with
 * the previous sub-step's damping fused in.  The last sub-step's damping is its own kernel.
 * reps = 1 is exactly one sub-step followed by its damping.
 * Returns the average time per sub-step in *ms_out.  ms_kernels[3] (may be NULL) gets
 * {edge phases, cell phases, the standalone damping}, each summed and divided by reps. */
int mpas_dyc_time_acoustic_step(mpas_dyc_ctx* ctx, double dts, int32_t small_step, int32_t reps,
                                double* ms_out, double* ms_kernels);
/* Capture one full timestep in a hipGraph and replay it for subsequent
 * mpas_dyc_timestep calls (1 = on, 0 = off). */
int mpas_dyc_use_graph(mpas_dyc_ctx* ctx, int32_t on);
/* Algorithmic HBM bytes of one acoustic sub-step of block 0 (B_ac). */
double mpas_dyc_acoustic_bytes(const mpas_dyc_ctx* ctx);
/* Exchange profile of a multi-rank run (bench.py --gpus N): with on = 1 every following
 * mpas_dyc_timestep runs eagerly (no hipGraph) with HIP events around the exposed part of each
 * halo exchange -- a blocking exchange whole, a split-phase one from the moment the compute stream
 * reaches the join until the exchange stream's work has completed -- and around each RCCL group.
 * mpas_dyc_get_profile then returns, for the last such step: out[0] = exchanges waited on,
 * out[1] = ms of the step (events on the compute stream), out[2] = ms of exposed exchange time,
 * out[3] = RCCL groups issued, out[4] = ms inside them (mostly overlapped with compute).
 * out[5] (profile on or off) = steps captured into a hipGraph since the context was created: it
 * stays put while steps replay (one capture per buffer layout and IAU branch, mpas_dyc_set_iau).
 * out[6] = ms of the last mpas_dyc_diag_update called with the profile on (HIP events around its
 * launches on the compute stream; that call is synchronous).
 * out[7] = the same for the last mpas_dyc_microphysics called with the profile on.
 * out[8] = the same for the last mpas_dyc_isobaric_diagnostics called with the profile on (written
 * only when n covers it, like every slot).
 * out[9] = the same for the last mpas_dyc_pv_diagnostics called with the profile on (its read-backs
 * included); out[10] = the sweeps of the last mpas_dyc_pv_diagnostics' fill that changed something, the
 * most over the blocks.
 * out[11] = milliseconds of the last mpas_dyc_convective_diagnostics called with the profile on.
 * out[12] = the same for the last mpas_dyc_physics_get_tend called with the profile on.
 * out[13] = the same for the last mpas_dyc_pv_budget_diagnostics called with the profile on (the PV
 * diagnostics it runs first included). */
int mpas_dyc_set_profile(mpas_dyc_ctx* ctx, int32_t on);
int mpas_dyc_get_profile(mpas_dyc_ctx* ctx, double* out, int32_t n);
/* The plan key of the exchange whose RCCL group was enqueued last ("warm_rccl <key>" while the
 * connections are set up before graph capture, which synchronises after every group): what a
 * watchdog reports when a rank hangs in RCCL.  Safe to read from another thread (a fixed buffer). */
const char* mpas_dyc_last_exchange(const mpas_dyc_ctx* ctx);
/* ncclGetVersion of the RCCL the library links (e.g. 22703 = 2.27.3), -1 on error. */
int32_t mpas_dyc_rccl_version(void);
/* How the kernels see a block, once its mesh is set (computed on the first call that needs it):
 * out[0] = maxEdges the kernels index with (max(nEdgesOnCell), at least 6 -- mesh files may
 * declare more, e.g. 10, Registry.xml:13-16), out[1] = maxEdges2 likewise, out[2] = kernel
 * family (0 one column per element, 1 batched stencil records, 2 pair layout: two elements per
 * wavefront, two levels per lane -- one element per wavefront above MPAS_DYC_MAX_LEVELS_WAVE,
 * one per workgroup of 128..256 lanes above MPAS_DYC_MAX_LEVELS_WIDE),
 * out[3] = column shape (0 one wavefront, 1 nVertLevels > MPAS_DYC_MAX_LEVELS_WAVE: one 128-lane
 * workgroup per column in the per-cell kernels, one wavefront per column in the pair layout; 2
 * nVertLevels > MPAS_DYC_MAX_LEVELS_WIDE: one workgroup per column in every kernel, of 256 lanes, 3
 * 512, 4 192, 5 320, 6 384, 7 448 lanes). */
int mpas_dyc_block_layout(mpas_dyc_ctx* ctx, int32_t block, int32_t* out /* [4] */);
/* Which Runge-Kutta stages of a step run their first acoustic cell phase in the launch of the
 * tendencies' last cell kernel (k_dyn_cells3_acoustic_r): bit 0 = stage 1, bit 1 = stage 2, bit 2 =
 * stage 3; 0 = none (several blocks or ranks, LBCs, more than 63 levels, a kernel family without
 * the per-cell records, or MPAS_DYCORE_FUSE_TEND_ACOUSTIC=0).  A first stage of several sub-steps
 * (order 2 with four or more) keeps the two kernels.  Valid once the mesh is set. */
int mpas_dyc_fused_tend_acoustic(mpas_dyc_ctx* ctx);
/* Which passes of a step are folded into the kernels that produce their inputs:
 * bit 0 = the averaging of ruAvg / wwAvg over the dynamics substeps is done by stage 3's last
 * damping and cell phase, and k_substep_finish_v is not launched (split transport, one block
 * without exchanges or LBCs, the pair layout with the fused recoveries, at most 63 levels;
 * MPAS_DYCORE_FOLD_SUBSTEP_AVG=0 turns it off); bit 1 = stage 1's edge kernel also applies the
 * del4 term and forms the final tend_u, and k_dyn_edges_rk1b_b is not launched (the pair layout,
 * at most 63 levels, no vertical mixing of u; MPAS_DYCORE_FOLD_RK1_EDGES=0 turns it off);
 * bit 2 = the w recovery after a stage runs in the launch of the diagnostics' cell kernel
 * (k_recover3_diag_cells_b; split transport, one block without exchanges or LBCs, the pair layout,
 * at most 63 levels; MPAS_DYCORE_FUSE_RECOVER_DIAG=0 turns it off); bit 3 = the recoveries of
 * stages 1 and 2 store no ruAvg / wwAvg: the next stage forms both again without reading them, and
 * the transport and the substep averaging read stage 3's (the conditions of bit 0;
 * MPAS_DYCORE_SKIP_STAGE_AVG=0 turns it off); bit 4 = the acoustic cell phases form cofwr, a_tri
 * and gamma_tri in registers from the other coefficients, and of a dt's coefficient calls only the
 * last stores the three (every block count, LBC runs too; at most 63 levels, maxEdges 6 or 7).  Set
 * while the coefficient arrays are those of the context's last coefficient call: not before the
 * first step, and not after mpas_dyc_set_field / mpas_dyc_field_device_ptr of coftz, cofwz, cofwr,
 * cofwt, a_tri, alpha_tri, gamma_tri or cofrz, until the next step (MPAS_DYCORE_DERIVE_COEFS=0 turns
 * it off); bit 5 = the diagnostics' cell kernel forms vorticity, ke_vertex and pv_vertex of the
 * cell's vertices itself from u at the cell's edges and spokes and stores pv_vertex and vorticity,
 * k_diag_vertices_p is not launched and ke_vertex is not stored (one block without exchanges whose
 * cells are all owned, the pair layout, at most 63 levels, and a mesh on which every vertex slot i
 * of a cell touches the cell's edges i and i-1 and every vertex has three cells;
 * MPAS_DYCORE_FUSE_DIAG_VERTICES=0 turns it off).
 * 0 = none.  Valid once the mesh is set. */
int mpas_dyc_folded_passes(mpas_dyc_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MPAS_DYCORE_H */
