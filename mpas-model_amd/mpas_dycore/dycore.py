"""Host-side mirror of the reference dycore interface over the C ABI.

The reference's operator API is the Fortran module ``atm_time_integration``
(mpas_atm_time_integration.F): the core driver calls ``atm_timestep`` each
step (mpas_atm_core.F:873), ``atm_init_coupled_diagnostics`` and
``atm_compute_solve_diagnostics`` at init (mpas_atm_core.F:390,399), and
shifts state time levels after each step (mpas_atm_core.F:671).  ``Dycore``
exposes exactly those operations; fields are addressed by (pool, name,
timeLevel) as in ``mpas_pool_get_array`` (mpas_pool_routines.F:4282), and
travel as element-major numpy arrays (the transpose-free view of the Fortran
(K, n+1) memory image).  Errors raise ``DycoreError`` (the reference aborts
through MPAS_LOG_CRIT, mpas_log.F:612).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import fields as F
from .layout import LOC_N, to_fortran

STATE_INPUTS = ("u", "w", "scalars")
# what atm_mpas_init_block precomputes (mpas_atm_core.F:311-358, 927-1288; mpas_dyc_model_init) and what
# it reads beyond the dycore's own mesh fields
MODEL_INIT_OUT = ("invAreaCell", "invDvEdge", "invDcEdge", "invAreaTriangle", "edgesOnVertex_sign",
                  "edgesOnCell_sign", "zb_cell", "zb3_cell", "kiteForCell", "nAdvCellsForEdge", "advCellsForEdge",
                  "adv_coefs", "adv_coefs_3rd", "meshScalingDel2", "meshScalingDel4", "meshScalingRegionalCell",
                  "meshScalingRegionalEdge", "dss")
MODEL_INIT_IN = ("deriv_two", "zb", "zb3", "meshDensity", "areaCell", "areaTriangle")
# and mpas_rbf_interp_initialize + mpas_init_reconstruct (mpas_atm_core.F:408-409; mpas_dyc_init_reconstruct)
RECONSTRUCT_IN = ("xCell", "yCell", "zCell", "xEdge", "yEdge", "zEdge")
DIAG_INPUTS = ("theta", "rho", "rho_base", "theta_base")
_SKIP = set(STATE_INPUTS) | set(DIAG_INPUTS) | {"xCell", "yCell", "zCell", "xEdge", "yEdge", "zEdge", "xVertex",
                                                "yVertex", "zVertex",
                                                "latVertex", "lonVertex", "areaCell", "areaTriangle",
                                                "meshDensity", "indexToCellID", "deriv_two", "zb", "zb3",
                                                "w_velocity_max", "wind_speed_level1_max", "updraft_helicity_max",
                                                *F.MICROP_FIELD, *F.ISO_CELL_FIELDS, *F.ISO_VERTEX_FIELDS,
                                                *F.ISO_LEVEL_TABLES, *F.PV_OUTPUTS, *F.PV_MESH_INPUTS, *F.CONV_OUTPUTS,
                                                *F.PVB_FIELDS}


def _host_allgather_fn(group, nranks: int):
    """mpas_dyc_comm_init_host's all-gather over a torch.distributed group: every rank's bytes, in rank
    order (CPU tensors, so gloo carries them)."""
    import torch
    import torch.distributed as dist

    def fn(send, recv, nbytes, user):
        try:
            mine = torch.frombuffer(bytearray(C.string_at(send, nbytes)), dtype=torch.uint8) if nbytes else \
                torch.zeros(0, dtype=torch.uint8)
            outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(nranks)]
            dist.all_gather(outs, mine, group=group)
            buf = b"".join(bytes(o.numpy().tobytes()) for o in outs)
            C.memmove(recv, buf, len(buf))
            return 0
        except Exception:  # noqa: BLE001 -- reported to the library as a failed all-gather
            return 1

    return _lib.ALLGATHER_FN(fn)


class DycoreError(RuntimeError):
    pass


def _make_dims(cases, solves, moist_end):
    dims = (_lib.Dims * len(cases))()
    for d, c, sv in zip(dims, cases, solves):
        d.nCells, d.nEdges, d.nVertices = c["nCells"], c["nEdges"], c["nVertices"]
        d.nVertLevels, d.maxEdges, d.maxEdges2 = c["nVertLevels"], c["maxEdges"], c["maxEdges2"]
        d.num_scalars = c["num_scalars"]
        if sv is None:
            sv = (c["nCells"], c["nEdges"], c["nVertices"])
        d.nCellsSolve, d.nEdgesSolve, d.nVerticesSolve = (int(x) for x in sv)
        d.moist_start, d.moist_end, d.index_qv = 1, moist_end, 1
    return dims


def _install_lists(lib, h, blocks, placement, check, positional_rank=None, include_self=False):
    """Every block's send / receive lists (mpas_multihalo_exchange_list) into the context.
    positional_rank (this process's rank): the lists with other ranks go in as mpas_dmpar keeps them
    for tasks of several blocks -- positions in one buffer per task pair (decomp.positional_lists,
    mpas_dyc_set_exchange_positions); include_self: this rank's own block pairs too."""
    code = {"cell": _lib.CELL, "edge": _lib.EDGE, "vertex": _lib.VERTEX}
    if positional_rank is not None:
        from .decomp import positional_lists
        pos = positional_lists(blocks, placement, positional_rank, include_self=include_self)
        for ib, (b, lst) in enumerate(zip(blocks, pos)):
            for dname, loc, layer, pr, idx, p in lst:
                a = np.ascontiguousarray(idx + 1, dtype=np.int32)
                p = np.ascontiguousarray(p, dtype=np.int32)
                check(lib.mpas_dyc_set_exchange_positions(h, ib, code[loc], int(layer),
                                                          _lib.SEND if dname == "send" else _lib.RECV, int(pr),
                                                          a.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                                                          int(a.size)), "set_exchange_positions")
            for direction, lists in ((_lib.SEND, b.send), (_lib.RECV, b.recv)):
                for loc, layer, peer, idx in lists:
                    pr, pb = placement[peer]
                    if pr != positional_rank or include_self:
                        continue
                    a = np.ascontiguousarray(np.asarray(idx, dtype=np.int32) + 1)
                    check(lib.mpas_dyc_set_exchange_list(h, ib, code[loc], int(layer), direction, int(pr), int(pb),
                                                         a.ctypes.data_as(C.c_void_p), int(a.size)), "set_exchange_list")
        return
    for ib, b in enumerate(blocks):
        for direction, lists in ((_lib.SEND, b.send), (_lib.RECV, b.recv)):
            for loc, layer, peer, idx in lists:
                pr, pb = placement[peer]
                a = np.ascontiguousarray(np.asarray(idx, dtype=np.int32) + 1)
                check(lib.mpas_dyc_set_exchange_list(h, ib, code[loc], int(layer), direction, int(pr), int(pb),
                                                     a.ctypes.data_as(C.c_void_p), int(a.size)), "set_exchange_list")


def plan_exchanges(blocks: list, placement: dict, rank: int, nranks: int, dt: float, moist_end: int = 1,
                   overlap: bool | None = None, positional: bool = False,
                   p2p: bool = False, todynamics: int = 0) -> tuple[np.ndarray, list[str]]:
    """Dry run of the exchange planner for one rank, on the host (no GPU): the RCCL messages
    this rank posts over model init and one step on each time-level parity, and the plan key of
    every exchange call in issue order (mpas_dyc_plan_exchanges).  Messages are a structured array
    with fields point, direction (_lib.SEND / _lib.RECV), block, peer_rank, peer_block, count.
    p2p: as planned for the one-sided transfer (mpas_dyc_set_p2p; the same messages, every exchange
    blocking).  todynamics: the MPAS_DYC_TODYN_* mask of mpas_dyc_set_todynamics (its wind flags add the halo
    exchange of the raw wind tendencies to every step)."""
    lib = _lib.load()
    cases = [b.case for b in blocks]
    dims = _make_dims(cases, [b.solve for b in blocks], moist_end)
    cfg = _lib.make_config(cases[0]["config"])
    h = C.c_void_p()
    rc = lib.mpas_dyc_create_blocks(len(cases), dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(h))
    if rc != 0 or not h.value:
        raise DycoreError(f"mpas_dyc_create_blocks(HOST_ONLY) failed ({rc})")

    def check(r, what):
        if r != 0:
            msg = lib.mpas_dyc_last_error(h)
            raise DycoreError(f"{what} failed ({r}): {msg.decode() if msg else ''}")
    try:
        _install_lists(lib, h, blocks, placement, check, positional_rank=rank if positional else None)
        check(lib.mpas_dyc_set_overlap(h, -1 if overlap is None else int(bool(overlap))), "set_overlap")
        if p2p:
            check(lib.mpas_dyc_set_p2p(h, 1), "set_p2p")
        if todynamics:
            check(lib.mpas_dyc_set_todynamics(h, int(todynamics), 0, 0, 0, 0, 0), "set_todynamics")
        nm, kl = C.c_int64(), C.c_int64()
        lib.mpas_dyc_plan_exchanges(h, int(nranks), int(rank), float(dt), None, 0, C.byref(nm), None, 0,
                                    C.byref(kl))
        msgs = (_lib.PlanMsg * max(1, nm.value))()
        keys = C.create_string_buffer(kl.value)
        check(lib.mpas_dyc_plan_exchanges(h, int(nranks), int(rank), float(dt), msgs, nm.value, C.byref(nm), keys,
                                          kl.value, C.byref(kl)), "plan_exchanges")
        dt_msg = np.dtype([("point", "<i4"), ("direction", "<i4"), ("block", "<i4"), ("peer_rank", "<i4"),
                           ("peer_block", "<i4"), ("count", "<i8")], align=True)
        assert dt_msg.itemsize == C.sizeof(_lib.PlanMsg)
        arr = np.frombuffer(bytes(msgs), dtype=dt_msg)[:nm.value].copy()
        return arr, keys.value.decode().splitlines()
    finally:
        lib.mpas_dyc_destroy(h)


class Dycore:
    """The blocks of this process on one GPU (MPAS domain%blocklist).

    ``Dycore(case)`` is one block owning every element (the single-GPU path);
    ``Dycore.from_blocks(...)`` takes the blocks of a decomposition
    (``mpas_dycore.decomp``) and installs their exchange lists."""

    def __init__(self, case: dict | None = None, device: int = 0, solve: tuple | None = None, moist_end: int = 1,
                 _blocks: list | None = None, model_init: str = "host"):
        self.lib = _lib.load()
        cases = [case] if _blocks is None else [b.case for b in _blocks]
        solves = [solve] if _blocks is None else [b.solve for b in _blocks]
        self.cases = cases
        self.case = cases[0]
        self.K = self.case["nVertLevels"]
        self.ns = self.case["num_scalars"]
        self.nblocks = len(cases)
        self.nb = [{"cell": c["nCells"], "edge": c["nEdges"], "vertex": c["nVertices"]} for c in cases]
        self.n = self.nb[0]
        dims = _make_dims(cases, solves, moist_end)
        cfg = _lib.make_config(self.case["config"])
        h = C.c_void_p()
        rc = self.lib.mpas_dyc_create_blocks(len(cases), dims, C.byref(cfg), int(device), C.byref(h))
        if rc != 0 or not h.value:
            raise DycoreError(f"mpas_dyc_create_blocks failed ({rc})")
        self.h = h
        self._mesh_set = set()  # (block, name) of the mesh fields uploaded so far
        if model_init not in ("host", "device", "device_cr"):
            raise ValueError("model_init: 'host' (the case's precomputed arrays), 'device' (mpas_dyc_model_init with "
                             "the C library's x**0.25 / sin from the host) or 'device_cr' (correctly rounded on the device)")
        for ib, c in enumerate(cases):
            self._upload_case(c, ib, device_init=model_init != "host", host_libm=model_init == "device")
        if model_init != "host":
            cfg = self.case["config"]
            self._check(self.lib.mpas_dyc_model_init(self.h, int(bool(cfg.get("config_h_ScaleWithMesh", True))),
                                                     float(cfg["config_zd"]), float(cfg["config_xnutr"])),
                        "model_init")
            if all(n in c for c in cases for n in RECONSTRUCT_IN):
                self._check(self.lib.mpas_dyc_init_reconstruct(self.h), "init_reconstruct")

    @classmethod
    def from_blocks(cls, blocks: list, device: int = 0, moist_end: int = 1, placement: dict | None = None,
                    rank: int = 0, nranks: int = 1, comm_id: bytes | None = None, rccl_local: bool = False,
                    positional: bool = False, p2p: bool | None = None, host_group=None):
        """Blocks of this process (``decomp.decompose(..., parts=...)``) on one GPU.

        ``placement`` maps every block (part) id to (rank, local block index); by
        default all blocks live in this process, in the given order.  With
        ``nranks`` > 1, ``comm_id`` is the RCCL unique id created on rank 0.  ``p2p``: one-sided
        transfer between the ranks of the node (mpas_dyc_set_p2p; None = MPAS_DYCORE_P2P).
        ``host_group``: a torch.distributed process group (gloo) of the ranks instead of ``comm_id``: no
        RCCL communicator, the set-up all-gathers go through the group (mpas_dyc_comm_init_host) and
        every halo message through the one-sided transfer."""
        if placement is None:
            placement = {b.part: (0, i) for i, b in enumerate(blocks)}
        self = cls(device=device, moist_end=moist_end, _blocks=blocks)
        if comm_id is not None:
            idb = C.create_string_buffer(bytes(comm_id), len(comm_id))
            self._check(self.lib.mpas_dyc_comm_init(self.h, idb, len(comm_id), int(nranks), int(rank)), "comm_init")
        elif host_group is not None:
            self._host_allgather = _host_allgather_fn(host_group, int(nranks))  # kept alive with the context
            self._check(self.lib.mpas_dyc_comm_init_host(self.h, int(nranks), int(rank), self._host_allgather, None),
                        "comm_init_host")
        if rccl_local:
            self._check(self.lib.mpas_dyc_set_transport(self.h, 1), "set_transport")
        if p2p is not None:
            self._check(self.lib.mpas_dyc_set_p2p(self.h, int(bool(p2p))), "set_p2p")
        # positional: the lists with other ranks as mpas_dmpar keeps them for tasks of several blocks (with
        # rccl_local, this process's block pairs too) -- the Fortran drop-in's path
        _install_lists(self.lib, self.h, blocks, placement, self._check, positional_rank=rank if positional else None,
                       include_self=positional and rccl_local)
        return self

    def p2p_active(self) -> bool:
        """True while halo messages between ranks use the one-sided transfer (mpas_dyc_get_p2p)."""
        return bool(self.lib.mpas_dyc_get_p2p(self.h))

    def graph_active(self) -> bool:
        """True if the last step replayed its captured hipGraph (False: it ran eagerly)."""
        return bool(self.lib.mpas_dyc_graph_active(self.h))

    @staticmethod
    def comm_unique_id() -> bytes:
        lib = _lib.load()
        n = lib.mpas_dyc_comm_unique_id_bytes()
        buf = C.create_string_buffer(n)
        if lib.mpas_dyc_comm_unique_id(buf, n) != 0:
            raise DycoreError("mpas_dyc_comm_unique_id failed")
        return buf.raw

    def init_deriv_two(self, inputs, block: int = 0):
        """mpas_dyc_init_deriv_two: deriv_two's least-squares fits on the device into mesh.deriv_two,
        from the transcendental inputs init_atm.deriv_two_inputs(mesh) returns (xp, yp, sin_the,
        cos_the, each (nCells, maxEdges))."""
        nC, me = self.cases[block]["nCells"], self.cases[block]["maxEdges"]
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in inputs]
        if len(arrs) != 4 or any(a.shape != (nC, me) for a in arrs):
            raise ValueError(f"deriv_two inputs: four ({nC}, {me}) arrays")
        self._check(self.lib.mpas_dyc_init_deriv_two(self.h, block, *[a.ctypes.data_as(C.c_void_p) for a in arrs]),
                    "init_deriv_two")

    def init_zb(self, theta_adv_order: int = 3, block: int = 0):
        """mpas_dyc_init_zb: zb / zb3 on the device from the block's deriv_two and zgrid."""
        self._check(self.lib.mpas_dyc_init_zb(self.h, block, int(theta_adv_order)), "init_zb")

    # -------------------------------------------------------------- fields
    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.mpas_dyc_last_error(self.h)
            raise DycoreError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def set_raw(self, pool: str, name: str, fortran_image: np.ndarray, time_level: int = 1, block: int = 0):
        a = np.ascontiguousarray(fortran_image)
        if pool == "mesh":
            self._mesh_set.add((block, name))
        self._check(self.lib.mpas_dyc_set_block_field(self.h, block, pool.encode(), name.encode(), time_level,
                                                      a.ctypes.data_as(C.c_void_p), a.nbytes),
                    f"set {pool}.{name}")

    def set(self, pool: str, name: str, arr, time_level: int = 1, block: int = 0):
        """Upload an element-major array (0-based indices for index fields)."""
        self.set_raw(pool, name, to_fortran({**self.cases[block], name: arr}, name), time_level, block)

    def get_raw(self, pool: str, name: str, time_level: int = 1, block: int = 0) -> np.ndarray:
        """Download a field's Fortran memory image (flat, garbage slot included): set_raw's inverse."""
        nb = self.lib.mpas_dyc_block_field_bytes(self.h, block, pool.encode(), name.encode())
        if nb <= 0:
            raise DycoreError(f"unknown field {pool}.{name}")
        buf = np.empty(nb // 4, dtype=np.int32) if name in F.INT_FIELDS else np.empty(nb // 8, dtype=np.float64)
        self._check(self.lib.mpas_dyc_get_block_field(self.h, block, pool.encode(), name.encode(), time_level,
                                                      buf.ctypes.data_as(C.c_void_p), buf.nbytes),
                    f"get {pool}.{name}")
        return buf

    def get(self, pool: str, name: str, time_level: int = 1, block: int = 0) -> np.ndarray:
        """Download a real field as element-major (n, inner) numpy (garbage slot dropped)."""
        nb = self.lib.mpas_dyc_block_field_bytes(self.h, block, pool.encode(), name.encode())
        if nb <= 0:
            raise DycoreError(f"unknown field {pool}.{name}")
        buf = np.empty(nb // 4, dtype=np.int32) if name in F.INT_FIELDS else np.empty(nb // 8, dtype=np.float64)
        self._check(self.lib.mpas_dyc_get_block_field(self.h, block, pool.encode(), name.encode(), time_level,
                                                      buf.ctypes.data_as(C.c_void_p), buf.nbytes),
                    f"get {pool}.{name}")
        loc = _loc_of(pool, name)
        if loc is None:
            return buf
        n1 = self.nb[block][loc] + 1
        if name in ("scalars", "scalars_tend"):
            return buf.reshape(n1, self.K, self.ns)[:-1]
        return buf.reshape(n1, buf.size // n1)[:-1]

    def set_overlap(self, on: bool | None = None):
        """Split-phase exchanges (interior elements overlap the halo traffic): True / False,
        or None for the library's automatic choice (on when exchanges go through RCCL)."""
        self._check(self.lib.mpas_dyc_set_overlap(self.h, -1 if on is None else (1 if on else 0)), "set_overlap")

    def halo_exchange(self, pool: str, name: str, time_level: int = 1, layers=(1, 2, 3)):
        """mpas_dmpar_exch_halo_field(field, haloLayers) over the blocks of this process (and peers)."""
        mask = sum(1 << (l - 1) for l in layers)
        self._check(self.lib.mpas_dyc_halo_exchange(self.h, pool.encode(), name.encode(), time_level, mask),
                    f"halo_exchange {pool}.{name}")

    def _upload_case(self, case: dict, block: int = 0, device_init: bool = False, host_libm: bool = True):
        """device_init: leave atm_mpas_init_block's precompute to the device (mpas_dyc_model_init) --
        upload its inputs (the init file's deriv_two, zb, zb3, meshDensity, areaCell, areaTriangle)
        instead of the case's precomputed arrays."""
        device_rec = device_init and all(n in case for n in RECONSTRUCT_IN)  # else the case's coefficients
        if device_init:
            for name in MODEL_INIT_IN + (RECONSTRUCT_IN if device_rec else ()):
                self.set_raw("mesh", name, to_fortran(case, name), block=block)
            # the C library's meshDensity**0.25 and damping-layer sin, as the compiled reference gets them
            # (init_atm.model_init_libm): the device's precompute then has the reference's bits
            if host_libm:
                from .init_atm import model_init_libm
                lm = model_init_libm(case, case["config"])
                for name, a in lm.items():
                    self.set_raw("mesh", name, to_fortran({**case, name: a}, name), block=block)
        for name in case:
            if name in _SKIP or name in F.IAU_FIELD or name in F.TODYN_RAW or name in F.TODYN_EDGE or (device_init and name in MODEL_INIT_OUT) or (device_rec and name == "coeffs_reconstruct"):
                continue
            if name in F.LOCATION or name in F.VERTICAL_1D:
                if name in F.VERTICAL_1D:
                    self.set_raw("mesh", name, np.asarray(case[name], dtype=np.float64), block=block)
                else:
                    self.set_raw("mesh", name, to_fortran(case, name), block=block)
            elif name in F.SCALARS_0D:
                self.set_raw("mesh", name, np.asarray([case[name]], dtype=np.float64), block=block)
        for name in STATE_INPUTS:
            self.set_raw("state", name, to_fortran(case, name), 1, block)
        for name in DIAG_INPUTS:
            self.set_raw("diag", name, to_fortran(case, name), block=block)
        for name, field in F.IAU_FIELD.items():  # the analysis increments, when the case carries them
            if name in case:
                self.set_raw("tend_iau", field, to_fortran(case, name), block=block)
        for name in F.TODYN_RAW:  # the raw physics tendencies, when the case carries them
            if name in case:
                self.set_raw("tend_physics", name, to_fortran(case, name), block=block)

    # -------------------------------------------------------- operators
    def init_diagnostics(self, dt: float):
        """atm_init_coupled_diagnostics + atm_compute_solve_diagnostics (mpas_atm_core.F:387-404)."""
        self._check(self.lib.mpas_dyc_init_diagnostics(self.h, float(dt)), "init_diagnostics")

    def restart_diagnostics(self, dt: float):
        """Model init of a restart run (config_do_restart, mpas_atm_core.F:387-404): only
        atm_compute_solve_diagnostics, on a coupled state the host has set (mpas_dyc_solve_diagnostics)."""
        self._check(self.lib.mpas_dyc_solve_diagnostics(self.h, float(dt)), "solve_diagnostics")

    def atm_timestep(self, dt: float, itimestep: int = 1):
        """atm_timestep -> atm_srk3 (mpas_atm_time_integration.F:87-139); asynchronous."""
        self._check(self.lib.mpas_dyc_timestep(self.h, float(dt), int(itimestep)), "atm_timestep")

    def set_lbc(self, apply: bool, seconds_to_interval_end: float = 0.0):
        """config_apply_lbcs (mpas_dyc_set_lbc): regional boundary conditions on/off, and before every
        step the seconds from the step's start to the end of the current LBC interval.  The driving
        data go into pool "lbc" (lbc_u, lbc_ru, lbc_rho_zz, lbc_rtheta_m, lbc_scalars; time level 1 =
        tendency, 2 = interval-end state) and the masks into the mesh pool."""
        self._check(self.lib.mpas_dyc_set_lbc(self.h, 1 if apply else 0, float(seconds_to_interval_end)), "set_lbc")

    PHYSICS_TENDENCIES, PHYSICS_RQVDYNTEN, PHYSICS_MICROPHYSICS = 1, 2, 4

    def set_physics(self, tendencies: bool = True, rqvdynten: bool = False, microphysics: bool = False):
        """Physics coupling (the reference's DO_PHYSICS build): the host sets tend_physics.
        tend_ru_physics / tend_rtheta_physics / tend_rho_physics and tend.scalars_tend before each
        step (as physics_get_tend does, mpas_atm_time_integration.F:424-449).  ``microphysics``: the
        host runs the microphysics on time level 2 after each step and then calls finish_step(),
        which runs the rest of atm_srk3 (the regional specified-zone reset, summarize_timestep)."""
        flags = ((self.PHYSICS_TENDENCIES if tendencies else 0) | (self.PHYSICS_RQVDYNTEN if rqvdynten else 0)
                 | (self.PHYSICS_MICROPHYSICS if microphysics else 0))
        self._check(self.lib.mpas_dyc_set_physics(self.h, flags), "set_physics")

    def set_iau(self, on: bool, window_length_s: float = 21600.0):
        """config_IAU_option / config_IAU_window_length_s (mpas_dyc_set_iau): the incremental analysis
        update of atm_srk3 (mpas_atm_iau.F).  The increments are the ``tend_iau`` pool -- ``u``, ``theta``,
        ``rho``, ``scalars`` through set / set_raw, or a case's ``u_amb``, ``theta_amb``, ``rho_amb``,
        ``scalars_amb`` (mpas_files.read_iau), which the constructor uploads.  Steps with itimestep <=
        nint(window_length_s / dt) are forced.  While on, the step runs as with
        set_physics(tendencies=True), with zero tendencies if the host supplies none."""
        self._check(self.lib.mpas_dyc_set_iau(self.h, 1 if on else 0, float(window_length_s)), "set_iau")

    def iau_weight(self, dt: float, itimestep: int) -> float:
        """atm_iau_coef (mpas_atm_iau.F:22-78): the weight of step ``itimestep``, 0.0 outside the
        window or with IAU off."""
        w = C.c_double()
        self._check(self.lib.mpas_dyc_iau_weight(self.h, float(dt), int(itimestep), C.byref(w)), "iau_weight")
        return w.value

    def graph_captures(self) -> int:
        """Steps captured into a hipGraph since the context was created (mpas_dyc_get_profile out[5])."""
        out = (C.c_double * 6)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 6), "get_profile")
        return int(out[5])

    DIAG_FIELDS = ("w_velocity_max", "wind_speed_level1_max", "updraft_helicity_max")

    @staticmethod
    def _diag_flags(w_max: bool, wsp_max: bool, uh_max: bool) -> int:
        return ((_lib.DIAG_W_VELOCITY_MAX if w_max else 0) | (_lib.DIAG_WIND_SPEED_LEVEL1_MAX if wsp_max else 0)
                | (_lib.DIAG_UPDRAFT_HELICITY_MAX if uh_max else 0))

    def set_diag_update(self, w_max: bool = True, wsp_max: bool = True, uh_max: bool = True, flags: int | None = None):
        """Which convective running maxima diag_update() advances (mpas_dyc_set_diag_update; the
        reference's is_needed_w_max / is_needed_lml_wsp_max / is_needed_updraft_helicity):
        ``diag.w_velocity_max``, ``diag.wind_speed_level1_max``, ``diag.updraft_helicity_max``, one value
        per cell, zero until updated or set (a restart puts them back with set()).  ``flags``: the
        MPAS_DYC_DIAG_* mask itself instead of the three switches.  The updraft helicity divides by
        areaCell, which the step itself never reads: it is uploaded here from the case."""
        if flags is None:
            flags = self._diag_flags(w_max, wsp_max, uh_max)
        self._check(self.lib.mpas_dyc_set_diag_update(self.h, int(flags)), "set_diag_update")
        if flags & _lib.DIAG_UPDRAFT_HELICITY_MAX:
            for ib, c in enumerate(self.cases):
                if "areaCell" in c:
                    self.set_raw("mesh", "areaCell", to_fortran(c, "areaCell"), block=ib)

    def diag_update(self):
        """mpas_atm_diag_update -> convective_diagnostics_update (convective_diagnostics.F:99-198) on the
        owned cells of every block, from w of time level 1 and the vorticity and reconstructed winds
        the last step left: call it after shift_time_levels().  Asynchronous; never part of the
        step's captured graph.  mpas_dycore.convective.update is its numpy restatement."""
        self._check(self.lib.mpas_dyc_diag_update(self.h), "diag_update")

    def diag_reset(self, w_max: bool = True, wsp_max: bool = True, uh_max: bool = True, flags: int | None = None):
        """convective_diagnostics_reset (:501-525), after a history write: the named maxima back to 0.0
        over the whole array (mpas_dyc_diag_reset)."""
        if flags is None:
            flags = self._diag_flags(w_max, wsp_max, uh_max)
        self._check(self.lib.mpas_dyc_diag_reset(self.h, int(flags)), "diag_reset")

    MICROP_SCHEMES = {None: _lib.MICROP_OFF, "off": _lib.MICROP_OFF, "kessler": _lib.MICROP_KESSLER}

    def field_bytes(self, pool: str, name: str, block: int = 0) -> int:
        """Bytes of a field's Fortran image (mpas_dyc_field_bytes); 0 for an unknown field and for the
        device microphysics' fields of a context that never asked for them."""
        return int(self.lib.mpas_dyc_block_field_bytes(self.h, block, pool.encode(), name.encode()))

    def set_microphysics(self, scheme: str | None = "kessler", index_qc: int = 2, index_qr: int = 3,
                         bucket_rainnc: float = 0.0):
        """config_microp_scheme on the device (mpas_dyc_set_microphysics).  ``"kessler"``: every
        atm_timestep runs driver_microphysics for mp_kessler on time level 2 inside the step (after the
        negative-scalar clip, before the regional reset and summarize_timestep; captured with the step),
        so the host neither downloads nor uploads the moist state.  ``index_qc`` / ``index_qr``: the
        1-based scalar indices of cloud and rain water; ``bucket_rainnc``: config_bucket_rainnc.  It
        keeps ``diag_physics`` rainnc / rainncv / precipw / i_rainnc, ``diag.surface_pressure`` and
        ``tend.tend_sfc_pressure`` (zero until updated or set; a restart puts rainnc, i_rainnc and
        surface_pressure back with set()).  While on, the step runs as with set_physics(tendencies=True)
        and reads tend.rt_diabatic_tend.  ``None`` / ``"off"``: off again.  Not together with
        set_physics(microphysics=True).  mpas_dycore.kessler.driver is its host restatement."""
        if scheme not in self.MICROP_SCHEMES and not isinstance(scheme, int):
            raise ValueError(f"unknown microphysics scheme {scheme!r} (Thompson and WSM6 stay with the host)")
        code = scheme if isinstance(scheme, int) and not isinstance(scheme, bool) else self.MICROP_SCHEMES[scheme]
        self._check(self.lib.mpas_dyc_set_microphysics(self.h, int(code), int(index_qc), int(index_qr),
                                                       float(bucket_rainnc)), "set_microphysics")

    def microphysics(self, dt: float, time_level: int = 2):
        """The scheme of set_microphysics once, eagerly and on its own, on ``time_level``
        (mpas_dyc_microphysics): for tests and hosts that sequence the step themselves.  Asynchronous."""
        self._check(self.lib.mpas_dyc_microphysics(self.h, float(dt), int(time_level)), "microphysics")

    def microphysics_ms(self, dt: float, time_level: int = 2) -> float:
        """Milliseconds of one microphysics() call between HIP events (mpas_dyc_get_profile out[7]);
        synchronous.  The call advances the fields like any other."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.microphysics(dt, time_level)
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 8)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 8), "get_profile")
        return float(out[7])

    def set_isobaric(self, flags: int | None = None, **groups: bool):
        """Which isobaric diagnostics isobaric_diagnostics() computes (mpas_dyc_set_isobaric; the
        reference's NEED_* switches, isobaric_diagnostics.F:96-259).  ``flags``: the MPAS_DYC_ISO_* mask
        (default: all), or keyword switches named like the constants of ``_lib`` without the prefix, e.g.
        ``set_isobaric(temperature=True, mslp=True)``.  A non-zero mask allocates, zeroed, the diag
        fields ``<group>_{200,250,500,700,850,925}hPa`` (vorticity_*hPa per vertex), ``mslp``,
        ``meanT_500_300``, ``t_isobaric`` (5 per cell), ``z_isobaric`` (13 per cell), the level tables
        ``t_iso_levels`` / ``z_iso_levels`` with the reference's constants, and the input ``relhum``
        (K per cell; the host's compute_relhum sets it, 0.0 until then).  The vorticity group divides by
        areaTriangle, which the step itself never reads: it is uploaded here from the case."""
        if groups:
            if flags is not None:
                raise ValueError("set_isobaric: either flags or keyword switches")
            flags = 0
            for name, on in groups.items():
                bit = getattr(_lib, "ISO_" + name.upper(), None)
                if bit is None or name.upper() == "ALL":
                    raise ValueError(f"set_isobaric: unknown group {name!r}")
                flags |= bit if on else 0
        elif flags is None:
            flags = _lib.ISO_ALL
        self._check(self.lib.mpas_dyc_set_isobaric(self.h, int(flags)), "set_isobaric")
        if flags & _lib.ISO_VORTICITY:
            for ib, c in enumerate(self.cases):
                if "areaTriangle" in c:
                    self.set_raw("mesh", "areaTriangle", to_fortran(c, "areaTriangle"), block=ib)

    def isobaric_diagnostics(self, time_level: int = 1):
        """interp_diagnostics (isobaric_diagnostics.F:265-895) on the owned cells and vertices of every
        block with the mask of set_isobaric (mpas_dyc_isobaric_diagnostics), from w, theta_m and qv of
        ``time_level``, diag.exner / pressure_p / pressure_base / relhum and the vorticity and
        reconstructed winds the last step left: call it after shift_time_levels().  Asynchronous; never
        part of the step's captured graph.  With the vorticity group on blocks that have exchange lists it
        first exchanges the halo of diag.pressure_p: collective across ranks.  mpas_dycore.isobaric is
        its numpy restatement."""
        self._check(self.lib.mpas_dyc_isobaric_diagnostics(self.h, int(time_level)), "isobaric_diagnostics")

    def isobaric_diagnostics_ms(self, time_level: int = 1) -> float:
        """Milliseconds of one isobaric_diagnostics() call between HIP events (mpas_dyc_get_profile
        out[8]); synchronous."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.isobaric_diagnostics(time_level)
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 9)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 9), "get_profile")
        return float(out[8])

    def set_pv(self, on: bool = True):
        """The switch of pv_diagnostics() (mpas_dyc_set_pv).  On: allocates, zeroed, diag.ertel_pv (K per
        cell), iLev_DT (int32), u_pv, v_pv, theta_pv, vort_pv and the three mesh vector arrays, which are
        uploaded here: the case's cellTangentPlane / localVerticalUnitVectors / edgeNormalVectors, or what
        reconstruct.initialize_vectors (mpas_initialize_vectors) makes of its cell centres; and areaCell,
        which the step itself never reads.  An edge of a block's outermost halo that lacks one of its cells
        in the block gets no meaningful normal; no owned cell has such an edge."""
        self._check(self.lib.mpas_dyc_set_pv(self.h, int(bool(on))), "set_pv")
        if not on:
            return
        from .reconstruct import initialize_vectors
        for ib, c in enumerate(self.cases):
            with np.errstate(invalid="ignore"):
                vec = c if all(n in c for n in F.PV_MESH_INPUTS) else initialize_vectors(c) if "xCell" in c else {}
            for name in F.PV_MESH_INPUTS:
                if name in vec:
                    self.set_raw("mesh", name, to_fortran({**c, name: vec[name]}, name), block=ib)
            if "areaCell" in c:
                self.set_raw("mesh", "areaCell", to_fortran(c, "areaCell"), block=ib)

    def pv_diagnostics(self, time_level: int = 1):
        """atm_compute_pv_diagnostics (pv_diagnostics.F:1218-1289) on every block
        (mpas_dyc_pv_diagnostics): theta and rho on all cells, ertel_pv on the owned cells, the tropopause
        level iLev_DT by the flood fill over the block, and u_pv, v_pv, theta_pv, vort_pv on the owned cells,
        from w, theta_m, rho_zz and qv of ``time_level`` and the vorticity and reconstructed winds the last
        step left: call it after shift_time_levels().  Synchronous; never part of the step's captured
        graph.  On blocks that have exchange lists it exchanges the halos of theta, uReconstructX/Y/Z, w and
        ertel_pv: collective across ranks.  mpas_dycore.pv is its numpy restatement."""
        self._check(self.lib.mpas_dyc_pv_diagnostics(self.h, int(time_level)), "pv_diagnostics")

    def pv_ms(self, time_level: int = 1) -> float:
        """Milliseconds of one pv_diagnostics() call between HIP events, the fill's read-backs included
        (mpas_dyc_get_profile out[9])."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.pv_diagnostics(time_level)
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 10)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 10), "get_profile")
        return float(out[9])

    def pv_sweeps(self) -> int:
        """Sweeps of the last pv_diagnostics()' fill that changed something, the most over the blocks
        (mpas_dyc_get_profile out[10])."""
        out = (C.c_double * 11)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 11), "get_profile")
        return int(out[10])

    def set_pv_budget(self, on: bool = True, lw: bool | None = None, sw: bool | None = None, bl: bool | None = None,
                      cu: bool | None = None, flags: int | None = None):
        """The switch of pv_budget_diagnostics() and the raw theta tendencies that are associated
        (mpas_dyc_set_pv_budget), after set_pv().  ``lw`` / ``sw`` / ``bl`` / ``cu``: rthratenlw / rthratensw /
        rthblten / rthcuten take part; None (the default) takes each from the schemes of set_todynamics (LW, SW,
        PBL -> bl, CU).  A source that is off gives exact zeros and is not read.  ``flags``: the MPAS_DYC_PVB_*
        mask itself.  On: allocates, zeroed, the diag fields of ``fields.PVB_FIELDS`` -- depv_dt_lw / sw / bl / cu /
        mp / mix / diab / fric, dtheta_dt_mp (the host's microphysics heating, an input) and dtheta_dt_mix (K per
        cell), depv_dt_diab_pv and depv_dt_fric_pv (one value per cell) -- and the library's scratch arrays; the
        curl divides by areaTriangle, which the step itself never reads: it is uploaded here from the case."""
        from . import pvbudget as B
        if flags is None:
            flags = 0
            if on:
                dflt = B.flags_from_todynamics(getattr(self, "_todyn_flags", 0))
                flags = B.ON
                for given, bit in ((lw, B.LW), (sw, B.SW), (bl, B.BL), (cu, B.CU)):
                    flags |= bit if (bool(dflt & bit) if given is None else given) else 0
        self._check(self.lib.mpas_dyc_set_pv_budget(self.h, int(flags)), "set_pv_budget")
        if flags:
            for ib, c in enumerate(self.cases):
                if "areaTriangle" in c:
                    self.set_raw("mesh", "areaTriangle", to_fortran(c, "areaTriangle"), block=ib)

    def pv_budget_diagnostics(self, time_level: int = 1):
        """atm_compute_pv_diagnostics and then atm_compute_pvBudget_diagnostics (pv_diagnostics.F:1291-1613) on every
        block (mpas_dyc_pv_budget_diagnostics): pv_diagnostics() unchanged, then dtheta_dt_mix on all cells and the
        eight depv_dt_* terms and their two values on the 2-PVU surface on the owned cells, from the raw theta
        tendencies of set_pv_budget, dtheta_dt_mp, tend_u_phys (0.0 without set_todynamics), tend.u_euler / w_euler
        / theta_euler and rho_edge as the last step left them: call it after shift_time_levels().  tend_u_phys and
        tend.w_euler keep their bits (the reference overwrites them).  Synchronous; never part of the step's captured
        graph; on blocks with exchange lists collective across ranks.  mpas_dycore.pvbudget is its numpy restatement."""
        self._check(self.lib.mpas_dyc_pv_budget_diagnostics(self.h, int(time_level)), "pv_budget_diagnostics")

    def pv_budget_ms(self, time_level: int = 1) -> float:
        """Milliseconds of one pv_budget_diagnostics() call between HIP events, pv_diagnostics() included
        (mpas_dyc_get_profile out[13])."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.pv_budget_diagnostics(time_level)
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 14)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 14), "get_profile")
        return float(out[13])

    def set_convective(self, flags: int | None = None, **outputs: bool):
        """Which outputs convective_diagnostics() computes (mpas_dyc_set_convective; the reference's
        MPAS_field_will_be_written switches, convective_diagnostics.F:285-312).  ``flags``: the
        MPAS_DYC_CONV_* mask (default: all), or keyword switches named like the constants of ``_lib``
        without the prefix, e.g. ``set_convective(cape=True, srh_0_3km=True)``.  A non-zero mask allocates,
        zeroed, the fourteen diag fields of ``fields.CONV_OUTPUTS``, one value per cell."""
        if outputs:
            if flags is not None:
                raise ValueError("set_convective: either flags or keyword switches")
            flags = 0
            for name, on in outputs.items():
                bit = getattr(_lib, "CONV_" + name.upper(), None)
                if bit is None or name.upper() == "ALL":
                    raise ValueError(f"set_convective: unknown output {name!r}")
                flags |= bit if on else 0
        elif flags is None:
            flags = _lib.CONV_ALL
        self._check(self.lib.mpas_dyc_set_convective(self.h, int(flags)), "set_convective")

    def convective_diagnostics(self, time_level: int = 1):
        """convective_diagnostics_compute (convective_diagnostics.F:227-487, with getcape) on the owned
        cells of every block with the mask of set_convective (mpas_dyc_convective_diagnostics), from
        theta_m and qv of ``time_level``, diag.exner / pressure_p / pressure_base and the reconstructed
        winds the last step left: call it after shift_time_levels().  With any bit the four *_surface
        fields are written; cape and cin come together; lcl and lfc are never written (the reference has
        no values for them).  Asynchronous; never part of the step's captured graph; not collective.
        mpas_dycore.convcompute is its numpy restatement."""
        self._check(self.lib.mpas_dyc_convective_diagnostics(self.h, int(time_level)), "convective_diagnostics")

    def convective_diagnostics_ms(self, time_level: int = 1) -> float:
        """Milliseconds of one convective_diagnostics() call between HIP events (mpas_dyc_get_profile
        out[11]); synchronous."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.convective_diagnostics(time_level)
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 12)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 12), "get_profile")
        return float(out[11])

    def set_todynamics(self, pbl: str | None = None, convection: str | None = None, lw=False, sw=False,
                       rqvdynten: bool = False, index_qc: int = 0, index_qr: int = 0, index_qi: int = 0,
                       index_qs: int = 0, index_ni: int = 0, flags: int | None = None):
        """physics_get_tend on the device (mpas_dyc_set_todynamics): every atm_timestep couples the raw
        tendencies of the ``tend_physics`` pool (``fields.TODYN_RAW``: rublten ... rthratensw, set through
        set / set_raw or written through the fields' device pointers, zero until then) into
        tend_ru_physics / tend_rtheta_physics / tend_rho_physics / scalars_tend, so the host uploads a raw
        tendency only when a scheme produced a new one.  ``pbl`` / ``convection``: config_pbl_scheme /
        config_convection_scheme by the reference's names (None or "off": none); ``lw`` / ``sw``:
        config_radt_lw_scheme / config_radt_sw_scheme is not 'off' (a bool, or the scheme's name);
        ``rqvdynten``: the step also computes tend_physics.rqvdynten.  ``index_q*`` / ``index_ni``: the
        1-based scalar indices, 0 for a scalar the run does not carry (its terms are skipped).  ``flags``:
        the MPAS_DYC_TODYN_* mask itself instead of the names.  Everything off: the hook is off.  Not together
        with set_physics(tendencies=True).  The wind tendencies are projected with ``mesh.east`` /
        ``mesh.north`` (the case's, uploaded by the constructor, or set()) and ``mesh.edgeNormalVectors`` (set(),
        or the case's, which is uploaded here if the block's has never been set); todynamics.with_vectors adds
        the three to a case.  Without them a step raises, naming the missing one.  mpas_dycore.todynamics is
        the numpy restatement."""
        from . import todynamics as T
        if flags is None:
            flags = T.scheme_flags(pbl, convection, lw, sw, rqvdynten)
        self._check(self.lib.mpas_dyc_set_todynamics(self.h, int(flags), int(index_qc), int(index_qr), int(index_qi),
                                                     int(index_qs), int(index_ni)), "set_todynamics")
        self._todyn_flags = int(flags)  # set_pv_budget's default sources
        if not flags & (T.PBL | T.CU_WINDS):
            return
        for ib, c in enumerate(self.cases):  # the constructor leaves the PV diagnostics' mesh vectors to their hooks
            if "edgeNormalVectors" in c and (ib, "edgeNormalVectors") not in self._mesh_set:
                self.set_raw("mesh", "edgeNormalVectors", to_fortran(c, "edgeNormalVectors"), block=ib)

    def physics_get_tend(self):
        """The coupling of set_todynamics once, eagerly and on its own, on time level 1
        (mpas_dyc_physics_get_tend): for hosts that want the coupled arrays, and for tests.  Asynchronous;
        collective across ranks when a wind tendency is projected (its halo exchange)."""
        self._check(self.lib.mpas_dyc_physics_get_tend(self.h), "physics_get_tend")

    def physics_get_tend_ms(self) -> float:
        """Milliseconds of one physics_get_tend() call between HIP events (mpas_dyc_get_profile out[12]);
        synchronous."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.physics_get_tend()
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 13)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 13), "get_profile")
        return float(out[12])

    def finish_step(self, dt: float):
        """The end of atm_srk3 after the host's microphysics (1672-1794); a no-op unless
        set_physics(microphysics=True).  Call before shift_time_levels."""
        self._check(self.lib.mpas_dyc_finish_step(self.h, float(dt)), "finish_step")

    def output_diagnostics(self, time_level: int = 1):
        """atm_compute_output_diagnostics (mpas_atm_core.F:753-800): diag theta, rho, pressure."""
        self._check(self.lib.mpas_dyc_output_diagnostics(self.h, int(time_level)), "output_diagnostics")

    def set_summary(self, global_minmax_vel: bool = True, detailed_minmax_vel: bool = False,
                    global_minmax_sca: bool = False):
        """The namelist switches of summarize_timestep (Registry.xml:339-349): which reductions
        every following step performs at its end (mpas_atm_time_integration.F:1794)."""
        flags = ((_lib.PRINT_GLOBAL_MINMAX_VEL if global_minmax_vel else 0)
                 | (_lib.PRINT_DETAILED_MINMAX_VEL if detailed_minmax_vel else 0)
                 | (_lib.PRINT_GLOBAL_MINMAX_SCA if global_minmax_sca else 0))
        self._check(self.lib.mpas_dyc_set_summary(self.h, flags), "set_summary")

    def summarize_timestep(self, log=None, block: int | None = None) -> dict:
        """summarize_timestep (mpas_atm_time_integration.F:6675-7018) of the last step: the global
        extrema over all blocks and ranks, and the reference's log lines (passed to ``log`` if given).
        ``block``: that block of this process only, reduced over ranks -- the reference writes one
        set of lines per block (6945-6983).
        In detailed mode a NaN in w or u raises DycoreError, as the reference aborts (6926-6940)."""
        s = _lib.Summary()
        mm = (C.c_double * (2 * self.ns))()
        if block is None:
            rc = self.lib.mpas_dyc_get_summary(self.h, C.byref(s), mm, 2 * self.ns)
        else:
            rc = self.lib.mpas_dyc_get_block_summary(self.h, int(block), C.byref(s), mm, 2 * self.ns)
        self._check(rc, "summarize_timestep")
        out = {"flags": s.flags, "w_min": s.w_min, "w_max": s.w_max, "u_min": s.u_min, "u_max": s.u_max,
               "nan_w": s.nan_w, "nan_u": s.nan_u, "scalars": [(mm[2 * i], mm[2 * i + 1]) for i in range(self.ns)]}
        for n in ("w_min_at", "w_max_at", "u_min_at", "u_max_at", "wsp_max_at"):
            e = getattr(s, n)
            out[n] = {"value": e.value, "k": e.k, "index": e.index, "lat": e.lat, "lon": e.lon}
        lines = []
        if s.flags & _lib.PRINT_DETAILED_MINMAX_VEL:
            lines.append("")
            for n, tag in (("w_min_at", "min w"), ("w_max_at", "max w"), ("u_min_at", "min u"),
                           ("u_max_at", "max u"), ("wsp_max_at", "max wsp")):
                e = out[n]
                lines.append(f" global {tag}: {e['value']} k={e['k']}, {e['lat']} lat, {e['lon']} lon")
        elif s.flags & _lib.PRINT_GLOBAL_MINMAX_VEL:
            lines += ["", f"global min, max w {s.w_min} {s.w_max}", f"global min, max u {s.u_min} {s.u_max}"]
        if s.flags & _lib.PRINT_GLOBAL_MINMAX_SCA:
            if not s.flags & (_lib.PRINT_GLOBAL_MINMAX_VEL | _lib.PRINT_DETAILED_MINMAX_VEL):
                lines.append("")
            lines += [f" global min, max scalar {i + 1} {a} {b}" for i, (a, b) in enumerate(out["scalars"])]
        out["log"] = lines
        if log is not None:
            for ln in lines:
                log(ln)
        if s.flags & _lib.PRINT_DETAILED_MINMAX_VEL and (s.nan_w or s.nan_u):
            raise DycoreError("NaN detected in '" + ("w" if s.nan_w else "u") + "' field.")
        return out

    def shift_time_levels(self):
        self._check(self.lib.mpas_dyc_shift_time_levels(self.h), "shift_time_levels")

    def synchronize(self):
        self._check(self.lib.mpas_dyc_synchronize(self.h), "synchronize")

    def use_graph(self, on: bool = True):
        self._check(self.lib.mpas_dyc_use_graph(self.h, 1 if on else 0), "use_graph")

    def time_acoustic_step(self, dts: float, small_step: int = 2, reps: int = 10):
        ms = C.c_double()
        ks = (C.c_double * 3)()
        self._check(self.lib.mpas_dyc_time_acoustic_step(self.h, float(dts), int(small_step), int(reps),
                                                         C.byref(ms), ks), "time_acoustic_step")
        return ms.value, list(ks)

    def layout(self, block: int = 0) -> dict:
        """How the kernels see a block (mpas_dyc_block_layout): the maxEdges / maxEdges2 they index
        with, the kernel family and the column shape ("wavefront": nVertLevels <= 63, a column per
        wavefront or half of one; "wide": 64..127, a wavefront per column in the pair layout, a
        128-lane workgroup in the per-cell kernels; "wide192": 128..191, a 192-lane workgroup per column
        in every kernel; "wide256": 192..255, a 256-lane workgroup; "wide320" / "wide384" / "wide448" /
        "wide512": up to 319 / 383 / 447 / 511 levels (MPAS_DYCORE_WIDE_TIGHT=0: 128..255 in 256 lanes,
        256..511 in 512).  Above 127 levels the pair-layout kernels keep two levels per lane over the
        workgroup's first 128 (192 / 256 lanes), 192 (320 / 384) or 256 (448 / 512) lanes."""
        out = (C.c_int32 * 4)()
        self._check(self.lib.mpas_dyc_block_layout(self.h, int(block), out), "block_layout")
        return {"maxEdges": out[0], "maxEdges2": out[1], "family": ("general", "batched", "pair")[out[2]],
                "column": ("wavefront", "wide", "wide256", "wide512", "wide192", "wide320", "wide384",
                           "wide448")[out[3]]}

    def fused_tend_acoustic(self) -> tuple:
        """The Runge-Kutta stages (1..3) whose first acoustic cell phase runs in the launch of the
        tendencies' last cell kernel (mpas_dyc_fused_tend_acoustic); () when none does: several
        blocks or ranks, LBCs, more than 63 levels, or MPAS_DYCORE_FUSE_TEND_ACOUSTIC=0."""
        m = int(self.lib.mpas_dyc_fused_tend_acoustic(self.h))
        return tuple(rk for rk in (1, 2, 3) if m & (1 << (rk - 1)))

    def folded_passes(self) -> tuple:
        """The passes this context folds into the kernels that produce their inputs
        (mpas_dyc_folded_passes): "substep_avg" -- stage 3's last damping and cell phase average
        ruAvg / wwAvg over the dynamics substeps and k_substep_finish_v is not launched
        (MPAS_DYCORE_FOLD_SUBSTEP_AVG=0: off); "rk1_edges" -- stage 1's edge kernel applies the del4
        term and forms the final tend_u and k_dyn_edges_rk1b_b is not launched
        (MPAS_DYCORE_FOLD_RK1_EDGES=0: off); "recover_diag" -- the w recovery runs in the launch of the
        diagnostics' cell kernel (MPAS_DYCORE_FUSE_RECOVER_DIAG=0: off); "stage_avg_stores" -- the
        recoveries of stages 1 and 2 store no ruAvg / wwAvg, which nothing reads before the next stage
        forms them again (MPAS_DYCORE_SKIP_STAGE_AVG=0: off); "derived_coefs" -- the acoustic cell phases
        form cofwr, a_tri and gamma_tri in registers and only the dt's last coefficient call stores
        them: reported while the coefficient arrays are those of this context's last coefficient call,
        so not before the first step and not after a set of one of them
        (MPAS_DYCORE_DERIVE_COEFS=0: off); "diag_vertices" -- the diagnostics' cell kernel forms its
        vertices' vorticity, ke_vertex and pv_vertex itself, k_diag_vertices_p is not launched and
        ke_vertex is not stored (one block, all cells owned, a mesh whose vertex slots follow the edge
        slots; MPAS_DYCORE_FUSE_DIAG_VERTICES=0: off).  () when none applies."""
        m = int(self.lib.mpas_dyc_folded_passes(self.h))
        names = ("substep_avg", "rk1_edges", "recover_diag", "stage_avg_stores", "derived_coefs", "diag_vertices")
        return tuple(n for i, n in enumerate(names) if m & (1 << i))

    def exchange_profile(self, dt: float, itimestep: int = 1) -> dict:
        """One eager atm_timestep with HIP events around every exchange's exposed part and every
        RCCL group (mpas_dyc_set_profile / mpas_dyc_get_profile); synchronous.  Shift the time
        levels afterwards as after any step."""
        self._check(self.lib.mpas_dyc_set_profile(self.h, 1), "set_profile")
        try:
            self.atm_timestep(dt, itimestep)
        finally:
            self._check(self.lib.mpas_dyc_set_profile(self.h, 0), "set_profile")
        out = (C.c_double * 5)()
        self._check(self.lib.mpas_dyc_get_profile(self.h, out, 5), "get_profile")
        return {"exchanges": int(out[0]), "ms_step_eager": out[1], "ms_exchange_exposed": out[2],
                "ms_compute": out[1] - out[2], "rccl_groups": int(out[3]), "ms_rccl_groups": out[4]}

    def last_exchange(self) -> str:
        """Plan key of the exchange whose RCCL group was enqueued last (thread-safe read)."""
        k = self.lib.mpas_dyc_last_exchange(self.h) if self.h else None
        return k.decode() if k else ""

    @staticmethod
    def rccl_version() -> int:
        return int(_lib.load().mpas_dyc_rccl_version())

    def acoustic_bytes(self) -> float:
        return self.lib.mpas_dyc_acoustic_bytes(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.mpas_dyc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# horizontal location of device fields not in fields.LOCATION
_LOCS = {}
for _n in ("theta_m", "rho_zz", "rho_p", "rtheta_p", "exner", "pressure_p", "pressure", "kdiff", "ke", "divergence", "rw",
           "wwAvg", "cqw", "h_divergence", "pv_cell", "rho_pp", "rtheta_pp", "rw_p", "exner_base", "pressure_base",
           "rtheta_base", "coftz", "cofwz", "cofwr", "cofwt", "a_tri", "alpha_tri", "gamma_tri", "rw_save",
           "tend_rtheta_adv", "rho_p_save", "rtheta_p_save", "rho_zz_old_split", "rtheta_pp_old", "wwAvg_split",
           "tend_rtheta_physics", "tend_rho_physics", "rqvdynten",
           "scalars_tend", "rthdynten", "rt_diabatic_tend", "theta_euler", "w_euler", "uReconstructX",
           "uReconstructY", "uReconstructZ", "uReconstructZonal", "uReconstructMeridional"):
    _LOCS[_n] = "cell"
for _n in ("ru", "ruAvg", "ru_p", "ru_save", "cqu", "rho_edge", "v", "pv_edge", "gradPVn", "gradPVt", "tend_ru_physics",
           "ruAvg_split", "u_euler"):
    _LOCS[_n] = "edge"
for _n in ("vorticity", "pv_vertex"):
    _LOCS[_n] = "vertex"


def _loc_of(pool: str, name: str):
    if pool == "tend" and name == "u":
        return "edge"
    if name in _LOCS:
        return _LOCS[name]
    return F.LOCATION.get(name)
