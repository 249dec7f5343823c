"""Drop-in for the parts of `BabelViscoFDTD.tools.RayleighAndBHTE` that BabelBrain's Step 2 uses
(imports at TranscranialModeling/BabelIntegrationBASE.py:19 and BabelIntegrationSingle.py:23):

    ForwardSimple(cwvnb, center, ds, u0, rf, deviceMetal=None)     Single:295, ANNULAR:383,411, CONCAVE:307,328,425,446
    ForwardSteered / ForwardElements                                not in the reference: its loops over steerings (CONCAVE:91-107)
                                                                   and over elements (H246:333-339, ANNULAR:379-384) as one call
    InitCuda / InitOpenCL / InitMetal(deviceName)                  BASE:918-925
    SpeedofSoundWater(T)                                           Single:243
    GenerateFocusTx(f, Foc, Diam, c, PPWSurface)                   Single:241

ForwardSimple runs on the MI355X through the C ABI (bfd_rayleigh_forward); there is no CPU fallback.
BHTE / BHTEMultiplePressureFields (CalculateTemperatureEffects.py:365-456, 960-990) run on the device too
(bfd_bhte_run_fields: four time steps per pass, csrc/bfd_bhte.hip). RunBHTECycles replaces the caller's own loop over them
(CalculateTemperatureEffects.py:259-460) with one device call for the whole protocol (bfd_bhte_run_protocol).
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _engine

_device = 0
_devices = None          # several HIP ordinals: ForwardSimple shares its field points among them (set_devices / BABELFDTD_DEVICES)
last_kernel_ms = None


def set_devices(devices):
    """Ordinals (or 'all') of the GPUs ForwardSimple may use together: the field points are independent, so they are dealt to
    the devices in contiguous shares, one host thread per device, no exchange (shard, no collective). None or
    one ordinal = single device. The environment variable BABELFDTD_DEVICES does the same for a caller that cannot pass
    arguments (the reference selects its device by name, BASE:918-925)."""
    global _devices, _device
    if devices is None:
        _devices = None
        return
    if isinstance(devices, str):
        devices = [d for d, _ in _engine.list_devices()] if devices.strip().lower() == 'all' else [int(x) for x in devices.split(',') if x.strip()]
    devices = [int(d) for d in devices]
    _devices = devices if len(devices) > 1 else None
    if len(devices) == 1:
        _device = devices[0]


def _init(deviceName=None):
    """Device selection by name substring, as the reference's Init* functions do (BASE:918-925)."""
    global _device
    devs = _engine.list_devices()
    if not devs:
        raise _engine.EngineError('no HIP device visible')
    if deviceName:
        for d, name in devs:
            if deviceName.lower() in name.lower():
                _device = d
                break
    return devs


InitCuda = InitOpenCL = InitMetal = InitMLX = InitHIP = _init      # the reference picks one by backend (BabelBrain.py:429-439)


def ForwardSimple(cwvnb, center, ds, u0, rf, deviceMetal=None, MacOsPlatform=None, u0step=0):
    """u2[n] = (i k / 2 pi) sum_m u0[m] ds[m] exp(-i k |rf[n]-center[m]|) / |rf[n]-center[m]|.
    cwvnb: complex wavenumber (Im k < 0 attenuates: the sum uses exp(-i k R) as written); center (M,3) f32; ds (M,) or (M,1) f32;
    u0 (M,) or (M,1) complex64; rf (N,3) f32. Returns complex64 (N,)."""
    global last_kernel_ms
    lib = _engine.load_library()
    k = complex(np.asarray(cwvnb).reshape(-1)[0])
    cen = np.ascontiguousarray(center, np.float32).reshape(-1, 3)
    a = np.ascontiguousarray(ds, np.float32).reshape(-1)
    u = np.ascontiguousarray(np.asarray(u0).reshape(-1), np.complex64)
    pts = np.ascontiguousarray(rf, np.float32).reshape(-1, 3)
    if not (len(a) == len(cen) == len(u)):
        raise ValueError('center, ds and u0 must describe the same number of sources')
    out = np.zeros(len(pts), np.complex64)
    devices = _devices
    if devices is None and os.environ.get('BABELFDTD_DEVICES'):
        set_devices(os.environ['BABELFDTD_DEVICES'])
        devices = _devices
    if devices is None or len(pts) < 64 * len(devices):
        devices = [_device]
    bounds = [len(pts) * r // len(devices) for r in range(len(devices) + 1)]
    times, errors = [0.0] * len(devices), [None] * len(devices)

    def share(r):          # ctypes releases the GIL for the call: the devices work at the same time
        n0, n1 = bounds[r], bounds[r + 1]
        if n1 <= n0:
            return
        ms = C.c_double()
        rc = lib.bfd_rayleigh_forward(devices[r], len(cen), cen.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                      u.view(np.float32).ctypes.data_as(C.c_void_p), k.real, k.imag, n1 - n0,
                                      pts[n0:n1].ctypes.data_as(C.c_void_p), out[n0:n1].view(np.float32).ctypes.data_as(C.c_void_p), C.byref(ms))
        if rc != 0:
            errors[r] = 'bfd_rayleigh_forward failed on device %d (rc=%d): %s' % (devices[r], rc, lib.bfd_last_error().decode())
        times[r] = ms.value
    if len(devices) == 1:
        share(0)
    else:
        th = [threading.Thread(target=share, args=(r,)) for r in range(len(devices))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    for e in errors:
        if e:
            raise _engine.EngineError(e)
    last_kernel_ms = max(times)
    return out


def _elem_start(elemdims, nSrc):
    """elemStart (int64, nElem + 1) of the records of each element: elemdims is one count for every element (CONCAVE's
    self._Tx['elemdims']: nSrc must be a multiple of it) or one count per element, flat or in the reference's
    elemdims[n][0] shape (H246:333-339, ANNULAR:379-384). The records of an element are contiguous, elements in
    ascending order (nBase += elemdims)."""
    if np.ndim(elemdims) == 0:
        c = int(elemdims)
        if c != elemdims or c <= 0 or nSrc % c:
            raise ValueError('a uniform elemdims must be a positive count that divides the %d sub-sources' % nSrc)
        counts = np.full(nSrc // c, c, np.int64)
    else:
        raw = np.asarray(elemdims)
        if raw.ndim == 2 and raw.shape[1] == 1:
            raw = raw[:, 0]
        if raw.ndim != 1 or (raw.size and not np.all(raw == np.floor(raw))):
            raise ValueError('elemdims must be an int or a sequence of counts (flat or [[c], ...])')
        counts = raw.astype(np.int64)
        if np.any(counts < 0):
            raise ValueError('elemdims holds a negative count')
        if counts.sum() != nSrc:
            raise ValueError('elemdims add up to %d, not to the %d sub-sources' % (counts.sum(), nSrc))
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]), np.int64)


def _forward_elements(cwvnb, center, ds, elemdims, weights, rf, u0):
    """ForwardSteered (weights (nElem, S)) and ForwardElements (weights None) through bfd_rayleigh_forward_elements; the field
    points are shared among the devices as in ForwardSimple."""
    global last_kernel_ms
    k = complex(np.asarray(cwvnb).reshape(-1)[0])
    cen = np.ascontiguousarray(center, np.float32).reshape(-1, 3)
    a = np.ascontiguousarray(ds, np.float32).reshape(-1)
    u = None if u0 is None else np.ascontiguousarray(np.asarray(u0).reshape(-1), np.complex64)
    pts = np.ascontiguousarray(rf, np.float32).reshape(-1, 3)
    if len(a) != len(cen) or (u is not None and len(u) != len(cen)):
        raise ValueError('center, ds and u0 must describe the same number of sources')
    es = _elem_start(elemdims, len(cen))
    nElem = len(es) - 1
    w = None
    if weights is not None:
        w = np.asarray(weights)
        if w.ndim == 1:
            w = w[:, None]
        if w.ndim != 2 or w.shape[0] != nElem:
            raise ValueError('weights must be (nElem, S) or (nElem,) with nElem = %d' % nElem)
        if w.shape[1] < 1:
            raise ValueError('weights must hold at least one steering column')
        w = np.ascontiguousarray(w, np.complex64)
    nOut = nElem if w is None else w.shape[1]
    lib = _engine.load_library()
    out = np.zeros((nOut, len(pts)), np.complex64)
    devices = _devices
    if devices is None and os.environ.get('BABELFDTD_DEVICES'):
        set_devices(os.environ['BABELFDTD_DEVICES'])
        devices = _devices
    if devices is None or len(pts) < 64 * len(devices):
        devices = [_device]
    bounds = [len(pts) * r // len(devices) for r in range(len(devices) + 1)]
    times, errors = [0.0] * len(devices), [None] * len(devices)

    def share(r):          # ctypes releases the GIL for the call: the devices work at the same time
        n0, n1 = bounds[r], bounds[r + 1]
        if n1 <= n0:
            return
        ms = C.c_double()
        part = out if len(devices) == 1 else np.empty((nOut, n1 - n0), np.complex64)
        rc = lib.bfd_rayleigh_forward_elements(devices[r], len(cen), _ptr(cen), _ptr(a), None if u is None else _ptr(u.view(np.float32)),
                                               nElem, _ptr(es), 0 if w is None else w.shape[1], None if w is None else _ptr(w.view(np.float32)),
                                               k.real, k.imag, n1 - n0, _ptr(pts[n0:n1]), _ptr(part.view(np.float32)), C.byref(ms))
        if rc != 0:
            errors[r] = 'bfd_rayleigh_forward_elements failed on device %d (rc=%d): %s' % (devices[r], rc, lib.bfd_last_error().decode())
            return
        if part is not out:
            out[:, n0:n1] = part
        times[r] = ms.value
    if len(devices) == 1:
        share(0)
    else:
        th = [threading.Thread(target=share, args=(r,)) for r in range(len(devices))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    for e in errors:
        if e:
            raise _engine.EngineError(e)
    last_kernel_ms = max(times)
    return out


def ForwardSteered(cwvnb, center, ds, elemdims, weights, rf, u0=None, deviceMetal=None):
    """S steered fields of a phased array over one geometry in one pass (bfd_rayleigh_forward_elements):
        out[s][n] = sum_e weights[e][s] (i k / 2 pi) sum_{m in element e} u0[m] ds[m] exp(-i k R_nm) / R_nm
    which is ForwardSimple with u0[m] -> weights[elem(m)][s] u0[m], for every column s, at about the cost of one such call: the
    reference runs its whole case once per MultiPoint entry (CONCAVE:91-107, ForwardSimple at :328 and :446) although only one
    complex number per element changes (:308-314). elemdims: records per element, an int (uniform, self._Tx['elemdims']) or a
    sequence of counts, flat or [[c], ...]; the records of an element are contiguous (nBase += elemdims). weights: (nElem, S) or
    (nElem,) complex; u0: optional per-sub-source factor (AdjustWeightAmplitudes, BASE:2224-2234), default 1.
    Returns complex64 (S, N). The field points are shared among several devices as in ForwardSimple."""
    if weights is None:
        raise ValueError('ForwardSteered needs weights (ForwardElements returns the element fields themselves)')
    return _forward_elements(cwvnb, center, ds, elemdims, weights, rf, u0)


def ForwardElements(cwvnb, center, ds, elemdims, rf, u0=None, deviceMetal=None):
    """The field of every element by itself, complex64 (nElem, N): row e is ForwardSimple on the records of element e alone
    (u0 default 1). One call for the per-element loops of H246:333-339, ANNULAR:379-384 and TxCalibration:323-328, 1021-1026;
    an empty element gives zeros. Arguments as in ForwardSteered."""
    return _forward_elements(cwvnb, center, ds, elemdims, None, rf, u0)


def SpeedofSoundWater(Temperature):
    """Speed of sound in pure water, m/s, Marczak (1997) fifth-order polynomial, 0-95 degC."""
    c = [2.787860e-9, -1.398845e-6, 3.287156e-4, -5.799136e-2, 5.038813, 1.402385e3]
    return np.polyval(c, Temperature)


def GenerateFocusTx(f, Foc, Diam, c, PPWSurface=4):
    """Spherical-cap radiator (apex at the origin, focus at z=+Foc) tessellated into patches of about
    lambda/PPWSurface: dict with 'center' (M,3), 'ds' (M,1), 'normal' (M,3), 'elemcenter' (1,3),
    'VertDisplay' (= centres) and the geometry scalars. Equal-area rings as in harness._bowl_points."""
    from .harness import _bowl_points
    lam = c / f
    amax = np.arcsin(min(Diam / 2 / Foc, 1.0))
    n_rings = max(int(np.ceil(Foc * amax / (lam / PPWSurface))), 4)
    pts, ds = _bowl_points(Foc, Diam, n_rings, 0.0)
    focus = np.array([[0.0, 0.0, Foc]])
    nrm = focus - pts
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return {'center': pts.astype(np.float32), 'ds': ds.reshape(-1, 1).astype(np.float32), 'normal': nrm.astype(np.float32),
            'elemcenter': np.zeros((1, 3), np.float32), 'VertDisplay': pts.astype(np.float32).copy(),
            'FaceDisplay': np.zeros((0, 4), np.int64), 'NumberElems': 1, 'Aperture': Diam, 'FocalLength': Foc}


# ------------------------------------------------------------------------------------------------
# BHTE: Pennes bio-heat equation + CEM43 dose on the device (bfd_bhte_run)
# ------------------------------------------------------------------------------------------------
# Heat source per voxel from the pressure amplitude. 'linear': Q = Absorption * alpha * p^2 / (rho c) (plane-wave intensity
# times the local absorption); 'exponential': the energy a plane wave loses crossing the voxel,
# Absorption * p^2 / (rho c) * (1 - exp(-2 h alpha)) / (2 h). They differ by about h*alpha (a few per cent in skull at
# 0.3-0.5 mm voxels). Which one the absent package uses is unverified; module-level default, per call
# through bhte_coefficients(source_form=...).
BHTE_SOURCE_FORM = 'linear'


def bhte_coefficients(MaterialList, dx, dt, DutyCycle=1.0, blood_rho=1050.0, blood_ct=3617.0, source_form=None):
    """Per-material float32 coefficients of the explicit scheme (documented in csrc/bfd_bhte.hip):
    cd = dt k/(rho c dx^2), cp = dt rho_b c_b w/(6e7 c) with w in mL/min/kg, and the factor qf that turns
    p^2 into the temperature increment of one ON step: qf = dt DutyCycle Absorption A/(rho^2 c_s c), A = Attenuation
    ('linear') or (1 - exp(-2 dx Attenuation))/(2 dx) ('exponential')."""
    rho = np.asarray(MaterialList['Density'], np.float64)
    ct = np.asarray(MaterialList['SpecificHeat'], np.float64)
    cd = dt * np.asarray(MaterialList['Conductivity'], np.float64) / (rho * ct * dx ** 2)
    cp = dt * blood_rho * blood_ct * np.asarray(MaterialList['Perfusion'], np.float64) / (6e7 * ct)
    att = np.asarray(MaterialList['Attenuation'], np.float64)
    form = BHTE_SOURCE_FORM if source_form is None else source_form
    if form == 'exponential':
        att = -np.expm1(-2.0 * dx * att) / (2.0 * dx)
    elif form != 'linear':
        raise ValueError("source_form must be 'linear' or 'exponential'")
    qf = (dt * DutyCycle * np.asarray(MaterialList['Absorption'], np.float64) * att
          / (rho * np.asarray(MaterialList['SoS'], np.float64)) / (rho * ct))
    if cd.max() > 1.0 / 6.0:
        raise ValueError('BHTE time step too large: dt k/(rho c dx^2) = %.3f > 1/6' % cd.max())
    return cd.astype(np.float32), cp.astype(np.float32), qf.astype(np.float32)


def field_schedule(nStepsOnOffList, TotalDurationSteps):
    """Which pressure field heats during each step: field n is on for nStepsOnOffList[n,0] steps, then nothing for
    nStepsOnOffList[n,1] steps, then field n+1 ...; the sequence repeats until TotalDurationSteps (the caller builds
    equal slots per focal spot, CalculateTemperatureEffects.py:715-736). -1 = no heating. Documented restatement:
    the package that defines it is absent from the reference tree."""
    oo = np.asarray(nStepsOnOffList, np.int64).reshape(-1, 2)
    if np.any(oo < 0) or oo.sum() <= 0:
        raise ValueError('nStepsOnOffList needs non-negative step counts and a non-empty cycle')
    cycle = np.concatenate([np.concatenate([np.full(on, n, np.int32), np.full(off, -1, np.int32)]) for n, (on, off) in enumerate(oo)])
    reps = -(-int(TotalDurationSteps) // len(cycle)) if TotalDurationSteps > 0 else 0
    return np.ascontiguousarray(np.tile(cycle, reps)[:int(TotalDurationSteps)], np.int32)


def bhte_pass_plan(sched, nFactorMonitoring=1, monitored_plane=True, steps_heating=4, steps_cooling=4, capture_steps=(), fuse=True):
    """The passes bfd_bhte_run_* cuts a schedule into: bhte_plan_passes of csrc/bfd_bhte_plan_core.h restated for byte accounting (tests/test_bhte_plan_host.py holds
    the two together, pass for pass). S steps per pass (4 by default) wherever the next S steps carry the same field and no capture boundary (capture_steps,
    ascending) lies strictly inside; else two steps where none lies between them, else one; fuse=False: every step on its own. Every pass kind is taken to fit
    the grid (fewer than 2^31 workgroups). Returns [(first step, length, heating)]."""
    sched = [int(v) for v in sched]
    caps = [int(c) for c in capture_steps]
    out, s, n, nxt = [], 0, len(sched), 0
    while s < n:
        while nxt < len(caps) and caps[nxt] == s:
            nxt += 1
        free = lambda L: nxt >= len(caps) or s + L <= caps[nxt]
        S = 2 if not fuse else steps_heating if sched[s] >= 0 else steps_cooling
        ok = 3 <= S <= 4 and s + S <= n and free(S) and all(sched[s + j] == sched[s] for j in range(1, S))
        L = S if ok else (2 if fuse and s + 1 < n and free(2) else 1)
        out.append((s, L, sched[s] >= 0 or (L == 2 and sched[s + 1] >= 0)))
        s += L
    return out


def _bhte_inputs(fields, MaterialMap, MaterialList, dx, dt, blood_rho, blood_ct, DutyCycle, MonitoringPointsMap, initT0, initDose):
    """Host-side checks and the arrays every bfd_bhte_run_* call takes (no device call). The width of the material ids follows from
    the LENGTH of MaterialList: up to 256 rows give a uint8 map for bfd_bhte_run_volumes / _protocol, more (a CT-derived list: up
    to 1030) a uint16 map for the ...16 entries; 'wide' says which."""
    P = np.asarray(fields)
    nF, N1, N2, N3 = P.shape
    mm = np.asarray(MaterialMap)
    nMat = len(MaterialList['Density'])
    if mm.shape != (N1, N2, N3):
        raise ValueError('MaterialMap must have the shape of the pressure field(s)')
    wide = nMat > 256
    bad_id = mm.size > 0 and (mm.min() < 0 or mm.max() >= nMat)
    if wide or bad_id:                  # the limit of the 16-bit path is the library's to say; up to 256 rows need no library here
        limit = int(_engine.load_library().bfd_bhte_max_materials())
        if nMat > limit:
            raise ValueError('MaterialList has %d rows: the bio-heat solver takes at most %d materials' % (nMat, limit))
        if bad_id:
            raise ValueError('MaterialMap ids must index MaterialList (%d rows; at most %d materials)' % (nMat, limit))
    cd, cp, qf = bhte_coefficients(MaterialList, dx, dt, DutyCycle, blood_rho, blood_ct)

    # The volumes go to the device in the caller's C order (bfd_bhte_run_volumes: last axis fastest, neighbours summed axis 0
    # first like the oracle does): no transposes; the heat source q = (p p) qf[material] is computed on the device and comes back.
    mat = np.ascontiguousarray(mm, np.uint16 if wide else np.uint8)     # every id < nMat (checked above): the cast cannot wrap
    P32 = np.ascontiguousarray(P, np.float32)
    flags = 0
    if initT0 is not None:
        T = np.array(initT0, np.float32, order='C'); flags |= 1
        if T.shape != (N1, N2, N3):
            raise ValueError('initT0 must have the shape of the pressure field')
    else:
        T = np.empty((N1, N2, N3), np.float32)
    if initDose is not None:
        dose = np.array(initDose, np.float32, order='C'); flags |= 2
        if dose.shape != (N1, N2, N3):
            raise ValueError('initDose must have the shape of the pressure field')
    else:
        dose = np.empty((N1, N2, N3), np.float32)
    initT = np.ascontiguousarray(MaterialList['InitTemperature'], np.float32)
    idx = None
    if hasattr(MonitoringPointsMap, 'ids') and hasattr(MonitoringPointsMap, 'indices'):
        # the sparse form (ThermalAnalysis.MonitoringPoints): the same rows as its dense map gives below, without a pass over the volume
        if tuple(MonitoringPointsMap.shape) != (N1, N2, N3):
            raise ValueError('MonitoringPointsMap must have the shape of the pressure field')
        ids, lin = np.asarray(MonitoringPointsMap.ids), np.asarray(MonitoringPointsMap.indices, np.int64)
        if ids.shape != lin.shape or ids.ndim != 1 or np.unique(lin).size != lin.size:
            raise ValueError('MonitoringPointsMap needs one id for each of its distinct linear indices')
        if lin.size and (lin.min() < 0 or lin.max() >= N1 * N2 * N3 or ids.min() == 0):
            raise ValueError('MonitoringPointsMap holds an index outside the volume or the id 0')
        idx = np.ascontiguousarray(lin[np.lexsort((lin, ids))], np.uint32)          # by id, then by linear index: flatnonzero, then the stable sort
    elif MonitoringPointsMap is not None:
        mp = np.asarray(MonitoringPointsMap)
        if mp.shape != (N1, N2, N3):
            raise ValueError('MonitoringPointsMap must have the shape of the pressure field')
        mp = mp.ravel()
        lin = np.flatnonzero(mp)
        order = np.argsort(mp[lin], kind='stable')               # point ids 1..n label the rows
        idx = np.ascontiguousarray(lin[order], np.uint32)
    return dict(shape=(nF, N1, N2, N3), nMat=nMat, wide=wide, mat=mat, cd=cd, cp=cp, qf=qf, initT=initT, P32=P32, T=T, dose=dose, flags=flags, idx=idx)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bhte_run(fields, sched, MaterialMap, MaterialList, dx, LocationMonitoring, nFactorMonitoring, dt, blood_rho, blood_ct,
              stableTemp, DutyCycle, MonitoringPointsMap, initT0, initDose):
    global last_kernel_ms
    lib = _engine.load_library()
    v = _bhte_inputs(fields, MaterialMap, MaterialList, dx, dt, blood_rho, blood_ct, DutyCycle, MonitoringPointsMap, initT0, initDose)
    nF, N1, N2, N3 = v['shape']
    T, dose, idx = v['T'], v['dose'], v['idx']
    q = np.empty((nF, N1, N2, N3), np.float32)
    nSteps = len(sched)
    fm = max(int(nFactorMonitoring), 1)
    slice_ok = LocationMonitoring is not None and int(LocationMonitoring) >= 0
    if slice_ok and int(LocationMonitoring) >= N2:
        raise ValueError('LocationMonitoring is outside the volume')
    nS = (nSteps + fm - 1) // fm if slice_ok else 0
    mon = np.zeros((N1, N3, nS), np.float32) if slice_ok else None
    pts = None if idx is None else np.zeros((len(idx), nSteps), np.float32)
    ms = C.c_double()
    sched = np.ascontiguousarray(sched, np.int32)
    if sched.size == 0:
        sched = np.full(1, -1, np.int32)

    ptr = _ptr
    entry = 'bfd_bhte_run_volumes16' if v['wide'] else 'bfd_bhte_run_volumes'
    rc = getattr(lib, entry)(_device, N1, N2, N3, v['nMat'], ptr(v['mat']), ptr(v['cd']), ptr(v['cp']), ptr(v['qf']), ptr(v['initT']), nF,
                             ptr(v['P32']), ptr(q), ptr(T), ptr(dose), v['flags'], float(stableTemp), float(dt), nSteps, ptr(sched),
                             int(LocationMonitoring) if slice_ok else -1, fm, ptr(mon), 0 if idx is None else len(idx), ptr(idx), ptr(pts), C.byref(ms))
    if rc != 0:
        raise _engine.EngineError('%s failed (rc=%d): %s' % (entry, rc, lib.bfd_last_error().decode()))
    last_kernel_ms = ms.value
    out = (T, dose, mon if slice_ok else np.zeros((0,), np.float32), q)
    if MonitoringPointsMap is not None:
        out = out + (pts,)
    return out


def BHTE(Pressure, MaterialMap, MaterialList, dx, TotalDurationSteps, nStepsOn, LocationMonitoring,
         nFactorMonitoring=1, dt=0.1, blood_rho=1050, blood_ct=3617, stableTemp=37.0, DutyCycle=1.0,
         Backend='HIP', MonitoringPointsMap=None, initT0=None, initDose=None):
    """Same call as the reference makes (CalculateTemperatureEffects.py:365-456, 960). Pressure: amplitude map
    (N1,N2,N3) Pa; MaterialMap: integer ids; MaterialList: dict of per-material arrays 'Density', 'SoS',
    'Attenuation' (Np/m), 'SpecificHeat', 'Conductivity', 'Perfusion' (mL/min/kg), 'Absorption' (fraction of the
    attenuation that heats), 'InitTemperature'. Returns (ResTemp, ResDose, MonitorSlice, Qarr[, TemperaturePoints])."""
    P = np.asarray(Pressure)
    if P.ndim != 3:
        raise ValueError('Pressure must be a 3-D amplitude map')
    nSteps = int(TotalDurationSteps)
    sched = np.full(nSteps, -1, np.int32)
    sched[:max(min(int(nStepsOn), nSteps), 0)] = 0
    out = _bhte_run(P[None], sched, MaterialMap, MaterialList, dx, LocationMonitoring, nFactorMonitoring, dt, blood_rho, blood_ct,
                    stableTemp, DutyCycle, MonitoringPointsMap, initT0, initDose)
    return out[:3] + (out[3][0],) + out[4:]


def BHTEMultiplePressureFields(PressureFields, MaterialMap, MaterialList, dx, TotalDurationSteps, nStepsOnOffList, LocationMonitoring,
                               nFactorMonitoring=1, dt=0.1, blood_rho=1050, blood_ct=3617, stableTemp=37.0, Backend='HIP',
                               MonitoringPointsMap=None, initT0=None, initDose=None):
    """Same call as the reference makes for steered multi-point sonications (CalculateTemperatureEffects.py:381-394,
    978-990): PressureFields (nFields,N1,N2,N3) Pa, nStepsOnOffList (nFields,2) int = steps on / off per field (see
    `field_schedule`). No DutyCycle argument: the on/off schedule is the duty cycle. Qarr comes back per field."""
    P = np.asarray(PressureFields)
    if P.ndim != 4:
        raise ValueError('PressureFields must be (nFields, N1, N2, N3)')
    oo = np.asarray(nStepsOnOffList).reshape(-1, 2)
    if oo.shape[0] != P.shape[0]:
        raise ValueError('nStepsOnOffList needs one (on, off) row per pressure field')
    sched = field_schedule(oo, int(TotalDurationSteps))
    return _bhte_run(P, sched, MaterialMap, MaterialList, dx, LocationMonitoring, nFactorMonitoring, dt, blood_rho, blood_ct,
                     stableTemp, 1.0, MonitoringPointsMap, initT0, initDose)


# ------------------------------------------------------------------------------------------------
# Repeated sonications (CalculateTemperatureEffects.py:259-460): the whole protocol as one device call (bfd_bhte_run_protocol)
# ------------------------------------------------------------------------------------------------
_MAX_STEPS = 2 ** 31 - 1


def protocol_schedule(nCurrent, Repetitions, TotalIterations, TotalDurationBetweenGroups, TotalDurationStepsOff,
                      LimitBHTEIterationsPerProcess, TotalDurationSteps, nStepsOn, multi_field=False, bRunInSubProcess=False):
    """The steps of the BHTE calls the reference's RunBHTECycles makes from iteration nCurrent on, back to back. Per iteration n:
    an ON call of TotalDurationSteps steps (one field: the first nStepsOn heat; several: field_schedule(nStepsOn,
    TotalDurationSteps), restarted at every ON call), then TotalDurationStepsOff cooling steps if that is > 0, then
    TotalDurationBetweenGroups cooling steps if (n + 1) % Repetitions == 0 and that is > 0. With bRunInSubProcess the run stops
    after the iteration where (n + 1) % LimitBHTEIterationsPerProcess == 0.
    Returns (fieldOfStep int32 [-1 = no heating], captureStep int32 [the step boundary at the end of each ON call], calls, nNext):
    calls lists (kind, n, first step, steps) per call, kind 'on' / 'off' / 'pause'; nNext is the iteration to resume from."""
    nCurrent, Repetitions, TotalIterations = int(nCurrent), int(Repetitions), int(TotalIterations)
    nOn, nOff, nPause = int(TotalDurationSteps), int(TotalDurationStepsOff), int(TotalDurationBetweenGroups)
    if Repetitions < 1:
        raise ValueError('Repetitions must be >= 1')
    if not 0 <= nCurrent < TotalIterations:
        raise ValueError('nCurrent must lie in [0, TotalIterations): there is no iteration to run')
    if nOn < 0 or nOff < 0 or nPause < 0:
        raise ValueError('step counts must be non-negative')
    nEnd = TotalIterations
    if bRunInSubProcess:
        limit = int(LimitBHTEIterationsPerProcess)
        if limit < 1:
            raise ValueError('LimitBHTEIterationsPerProcess must be >= 1')
        nEnd = min(TotalIterations, (nCurrent // limit + 1) * limit)
    calls, pos = [], 0
    for n in range(nCurrent, nEnd):
        calls.append(('on', n, pos, nOn)); pos += nOn
        if TotalDurationStepsOff > 0:
            calls.append(('off', n, pos, nOff)); pos += nOff
        if (n + 1) % Repetitions == 0 and TotalDurationBetweenGroups > 0:
            calls.append(('pause', n, pos, nPause)); pos += nPause
        if pos > _MAX_STEPS:
            raise ValueError('the protocol has more than 2^31 - 1 steps')
    if multi_field:
        on = field_schedule(nStepsOn, nOn)
    else:
        on = np.full(nOn, -1, np.int32)
        on[:max(min(int(nStepsOn), nOn), 0)] = 0
    fieldOfStep = np.full(pos, -1, np.int32)
    caps = []
    for kind, n, first, steps in calls:
        if kind == 'on':
            fieldOfStep[first:first + steps] = on
            caps.append(first + steps)
    return fieldOfStep, np.array(caps, np.int32), calls, nEnd


def RunBHTECycles(nCurrent, Repetitions, TotalIterations, TotalDurationBetweenGroups, TotalDurationStepsOff, LimitBHTEIterationsPerProcess,
                  InputPData, PMaps, MaterialMap, MaterialList, dx, TotalDurationSteps, nStepsOn, cy, nFactorMonitoring, dt, DutyCycle,
                  Backend, MonitoringPointsMap, stableTemp, TemperaturePoints, FinalTemp, FinalDose, PreviousData, bRunInSubProcess=False):
    """Drop-in for the caller's own loop (CalculateTemperatureEffects.py:259-460, driven at :1026-1100), same positional signature
    and return value (ResTempMax, ResDose, FinalTemp, FinalDose, TemperaturePoints, nCurrent_next). The loop's ON calls (BHTE
    when InputPData is a str: PMaps (N1,N2,N3), DutyCycle in the heat source; else BHTEMultiplePressureFields: PMaps
    (nF,N1,N2,N3), nStepsOn = nStepsOnOffList, duty cycle 1), OFF calls and group pauses run as ONE device call
    (bfd_bhte_run_protocol, schedule from `protocol_schedule`): T and the dose stay on the device, the temperature maximum over the
    ends of the ON calls and the dose at the last of them are taken there. Every output equals what the chain of BHTE calls gives.
    Start state: at nCurrent == 0 PreviousData['FinalTemp' / 'FinalDose'] if given, else InitTemperature[material] and zero dose;
    at nCurrent > 0 the FinalTemp / FinalDose passed in. TemperaturePoints is replaced at nCurrent == 0 and appended to otherwise.
    Resuming (nCurrent > 0, the bRunInSubProcess chunks of :1040-1105): ResTempMax is the maximum over the ON calls of THIS call
    -- the caller combines chunks with np.maximum (:1094-1098); the reference's own loop cannot resume (its ResTempMax is unbound
    there). cy (the monitored plane, which the caller discards: it passes -1) is ignored, and so is Backend (always the HIP device).
    MonitoringPointsMap is required, as the reference's unpacking of five returns needs it."""
    global last_kernel_ms
    single = isinstance(InputPData, str)
    P = np.asarray(PMaps)
    if single:
        if P.ndim != 3:
            raise ValueError('PMaps must be a 3-D amplitude map when InputPData is a file name')
        fields = P[None]
    else:
        if P.ndim != 4:
            raise ValueError('PMaps must be (nFields, N1, N2, N3) for steered fields')
        oo = np.asarray(nStepsOn)
        if oo.ndim != 2 or oo.shape != (P.shape[0], 2):
            raise ValueError('nStepsOnOffList needs one (on, off) row per pressure field')
        fields = P
    shape = fields.shape[1:]
    if np.shape(MaterialMap) != shape:
        raise ValueError('MaterialMap must have the shape of the pressure field(s)')
    if MonitoringPointsMap is None:
        raise ValueError('RunBHTECycles needs a MonitoringPointsMap')
    if np.shape(MonitoringPointsMap) != shape:
        raise ValueError('MonitoringPointsMap must have the shape of the pressure field')
    sched, caps, _, nNext = protocol_schedule(nCurrent, Repetitions, TotalIterations, TotalDurationBetweenGroups, TotalDurationStepsOff,
                                              LimitBHTEIterationsPerProcess, TotalDurationSteps, nStepsOn, not single, bRunInSubProcess)
    if int(nCurrent) > 0:
        initT0, initDose = FinalTemp, FinalDose
    elif PreviousData is not None:
        initT0, initDose = PreviousData['FinalTemp'], PreviousData['FinalDose']
    else:
        initT0 = initDose = None
    v = _bhte_inputs(fields, MaterialMap, MaterialList, dx, dt, 1050, 3617, DutyCycle if single else 1.0, MonitoringPointsMap, initT0, initDose)
    idx = v['idx']
    if int(nCurrent) > 0:
        if TemperaturePoints is None or np.ndim(TemperaturePoints) != 2 or np.shape(TemperaturePoints)[0] != len(idx):
            raise ValueError('TemperaturePoints must hold one row per monitoring point when resuming (nCurrent > 0)')
    nF, N1, N2, N3 = v['shape']
    nSteps = len(sched)
    pts = np.zeros((len(idx), nSteps), np.float32)
    Tmax = np.empty((N1, N2, N3), np.float32)
    doseCap = np.empty((N1, N2, N3), np.float32)
    T, dose = v['T'], v['dose']
    if nSteps == 0:
        sched = np.full(1, -1, np.int32)
    lib = _engine.load_library()
    ms = C.c_double()
    ptr = _ptr
    entry = 'bfd_bhte_run_protocol16' if v['wide'] else 'bfd_bhte_run_protocol'
    rc = getattr(lib, entry)(_device, N1, N2, N3, v['nMat'], ptr(v['mat']), ptr(v['cd']), ptr(v['cp']), ptr(v['qf']), ptr(v['initT']), nF,
                             ptr(v['P32']), None, ptr(T), ptr(dose), v['flags'], float(stableTemp), float(dt), nSteps, ptr(sched),
                             -1, max(int(nFactorMonitoring), 1), None, len(idx), ptr(idx), ptr(pts), C.byref(ms),
                             len(caps), ptr(caps), ptr(Tmax), ptr(doseCap))
    if rc != 0:
        raise _engine.EngineError('%s failed (rc=%d): %s' % (entry, rc, lib.bfd_last_error().decode()))
    last_kernel_ms = ms.value
    if int(nCurrent) > 0:
        pts = np.hstack((TemperaturePoints, pts))
    return Tmax, doseCap, T, dose, pts, nNext
