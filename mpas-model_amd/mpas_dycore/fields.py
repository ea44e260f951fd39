"""Field registry: MPAS names, pools, horizontal location and index semantics.

Names follow core_atmosphere/Registry.xml (var_struct mesh/state/diag/tend,
Registry.xml:1127-1779).  Arrays on the Python side are element-major numpy
arrays, e.g. ``u`` has shape (nEdges, K) -- the transpose of the Fortran
``u(K, nEdges+1)`` without the garbage slot -- so a row is one contiguous
column of K levels, exactly the layout used in HBM (k is the fast axis).
"""
from __future__ import annotations

# name -> horizontal location of the LEADING numpy axis
LOCATION = {}
for n in ("latCell lonCell xCell yCell zCell areaCell invAreaCell meshDensity nEdgesOnCell indexToCellID "
          "edgesOnCell cellsOnCell verticesOnCell kiteForCell edgesOnCell_sign defc_a defc_b zgrid zz dss "
          "zb_cell zb3_cell theta rho scalars rho_base theta_base w coeffs_reconstruct t_init "
          "bdyMaskCell nearestRelaxationCell meshScalingRegionalCell specZoneMaskCell "
          "meshDensity_root4 dss_sin").split():
    LOCATION[n] = "cell"
for n in ("latEdge lonEdge xEdge yEdge zEdge dcEdge dvEdge invDcEdge invDvEdge angleEdge fEdge "
          "meshScalingDel2 meshScalingDel4 nEdgesOnEdge nAdvCellsForEdge cellsOnEdge verticesOnEdge "
          "edgesOnEdge advCellsForEdge weightsOnEdge adv_coefs adv_coefs_3rd zxu deriv_two zb zb3 u "
          "bdyMaskEdge meshScalingRegionalEdge specZoneMaskEdge meshDensityEdge_root4").split():
    LOCATION[n] = "edge"
for n in ("latVertex lonVertex xVertex yVertex zVertex areaTriangle invAreaTriangle fVertex "
          "cellsOnVertex edgesOnVertex edgesOnVertex_sign kiteAreasOnVertex").split():
    LOCATION[n] = "vertex"

# index arrays -> which element set they point into (0-based in numpy, -1 = none)
INDEX_TARGET = {
    "edgesOnCell": "edge", "cellsOnCell": "cell", "verticesOnCell": "vertex",
    "cellsOnEdge": "cell", "verticesOnEdge": "vertex", "edgesOnEdge": "edge",
    "advCellsForEdge": "cell", "cellsOnVertex": "cell", "edgesOnVertex": "edge",
    "nearestRelaxationCell": "cell",
}
# small-integer arrays stored 0-based in numpy but 1-based in MPAS (not element indices)
ONE_BASED_SMALL = {"kiteForCell"}
COUNTS = {"nEdgesOnCell", "nEdgesOnEdge", "nAdvCellsForEdge", "indexToCellID"}

# the analysis increments of the incremental analysis update as a case carries them -> their field
# in the tend_iau pool (Registry.xml:3101-3132: name "tend_u", name_in_code "u", ...)
IAU_FIELD = {"u_amb": "u", "theta_amb": "theta", "rho_amb": "rho", "scalars_amb": "scalars"}
LOCATION.update(u_amb="edge", theta_amb="cell", rho_amb="cell", scalars_amb="cell")

# the convective running maxima of mpas_dyc_diag_update (diag pool, one value per cell)
LOCATION.update(w_velocity_max="cell", wind_speed_level1_max="cell", updraft_helicity_max="cell")

# the device microphysics' fields (mpas_dyc_set_microphysics): pool by name, one value per cell
MICROP_FIELD = {"rainnc": "diag_physics", "rainncv": "diag_physics", "precipw": "diag_physics",
                "i_rainnc": "diag_physics", "surface_pressure": "diag", "tend_sfc_pressure": "tend"}
LOCATION.update({n: "cell" for n in MICROP_FIELD})
INT_FIELDS = {"i_rainnc", "iLev_DT"}   # int32 on the device, not an index into an element set

# the isobaric diagnostics (mpas_dyc_set_isobaric; diag pool): <group>_<level>hPa per cell, vorticity_*hPa
# per vertex, mslp, meanT_500_300, t_isobaric (5 per cell), z_isobaric (13 per cell), the host's relhum (K per
# cell); t_iso_levels (5) and z_iso_levels (13) have no horizontal location
ISO_GROUPS = ("temperature", "relhum", "dewpoint", "uzonal", "umeridional", "height", "w", "vorticity")
ISO_HPA = (200, 250, 500, 700, 850, 925)
ISO_CELL_FIELDS = tuple(f"{g}_{p}hPa" for g in ISO_GROUPS[:-1] for p in ISO_HPA) + (
    "mslp", "meanT_500_300", "t_isobaric", "z_isobaric", "relhum")
ISO_VERTEX_FIELDS = tuple(f"vorticity_{p}hPa" for p in ISO_HPA)
ISO_LEVEL_TABLES = ("t_iso_levels", "z_iso_levels")
LOCATION.update({n: "cell" for n in ISO_CELL_FIELDS})
LOCATION.update({n: "vertex" for n in ISO_VERTEX_FIELDS})

# the PV diagnostics (mpas_dyc_set_pv): the outputs in the diag pool, one column (ertel_pv) or one value per
# cell, and the mesh vectors of mpas_initialize_vectors they read
PV_OUTPUTS = ("ertel_pv", "iLev_DT", "u_pv", "v_pv", "theta_pv", "vort_pv")
PV_MESH_INPUTS = ("cellTangentPlane", "localVerticalUnitVectors", "edgeNormalVectors")
LOCATION.update({n: "cell" for n in PV_OUTPUTS + PV_MESH_INPUTS[:2]})
LOCATION["edgeNormalVectors"] = "edge"

# the output-time convective diagnostics (mpas_dyc_set_convective; diag pool), one value per cell, in the bit
# order of MPAS_DYC_CONV_*
CONV_OUTPUTS = ("cape", "cin", "lcl", "lfc", "srh_0_1km", "srh_0_3km", "uzonal_surface", "uzonal_1km", "uzonal_6km",
                "umeridional_surface", "umeridional_1km", "umeridional_6km", "temperature_surface", "dewpoint_surface")
LOCATION.update({n: "cell" for n in CONV_OUTPUTS})

# physics_get_tend on the device (mpas_dyc_set_todynamics): the raw tendencies of the PBL, convection and
# radiation schemes (tend_physics pool, one column per cell), the edge projections of the wind tendencies
# (tend_physics) and diag.tend_u_phys (one column per edge), and init_dirs_forphys' mesh.east / north
TODYN_RAW = ("rublten", "rvblten", "rthblten", "rqvblten", "rqcblten", "rqiblten", "rniblten", "rucuten", "rvcuten",
             "rthcuten", "rqvcuten", "rqccuten", "rqrcuten", "rqicuten", "rqscuten", "rthratenlw", "rthratensw")
TODYN_EDGE = ("rublten_Edge", "rucuten_Edge", "tend_u_phys")
TODYN_MESH_INPUTS = ("east", "north")
LOCATION.update({n: "cell" for n in TODYN_RAW + TODYN_MESH_INPUTS})
LOCATION.update({n: "edge" for n in TODYN_EDGE})

# the PV budget (mpas_dyc_set_pv_budget; diag pool): the eight terms and the two heating rates, one column per
# cell (dtheta_dt_mp is the host's input), and the two terms on the 2-PVU surface, one value per cell
PVB_OUTPUTS_3D = ("depv_dt_lw", "depv_dt_sw", "depv_dt_bl", "depv_dt_cu", "depv_dt_mp", "depv_dt_mix", "depv_dt_diab",
                  "depv_dt_fric")
PVB_HEATING = ("dtheta_dt_mp", "dtheta_dt_mix")
PVB_OUTPUTS_2D = ("depv_dt_diab_pv", "depv_dt_fric_pv")
PVB_FIELDS = PVB_OUTPUTS_3D + PVB_HEATING + PVB_OUTPUTS_2D
LOCATION.update({n: "cell" for n in PVB_FIELDS})

VERTICAL_1D = ("fzm", "fzp", "rdzw", "rdzu", "u_init", "v_init")
SCALARS_0D = ("cf1", "cf2", "cf3")


def count_of(case: dict, loc: str) -> int:
    return {"cell": case["nCells"], "edge": case["nEdges"], "vertex": case["nVertices"]}[loc]
