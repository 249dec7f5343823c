"""Step 2 as one device-resident study: the label volume, the CT index volume and the air mask of TranscranialModeling/BabelIntegrationBASE.py
:1840-2201 are uploaded once; the material map is assembled, handed to the solver, and the results are scattered, scaled, cropped and flipped
(:2433-2520, :2729-2885) without leaving the MI355X until a volume is asked for (the bfd_acoustic handle of include/babelfdtd.h,
csrc/bfd_acoustic.hip).

    with AcousticStudy(labels, ct_index, air) as st:
        plan = st.plan(SpatialStep, FocalLength=..., Aperture=...)       Domain.plan_domain, its two surveys on the resident labels
        stats = st.assemble(plan, n_materials)                           Domain.assemble, the maps stay resident
        st.engine(MaterialList, Frequency, SpatialStep, dt, nt, ...)     Engine with sensorMode 1, the resident map and the sensor box attached
        st.set_source_plane(u0, T)                                       the complex plane at ZSourceLocation -> SeparableSource.cw
        st.run()
        st.pack(correction, slot=0)                                      Engine.pack_results into resident volumes, the maps with them
        d = st.data_for_sim(Material, zLengthBeyonFocalPoint)            results.data_for_sim, the volumes fetched

Every method runs the launch sequence of the public call it mirrors (Domain.survey / assemble, Engine.set_material_map / set_reflector /
set_sensor_map, Engine.pack_results), so its results equal theirs element by element. `acoustic_field` is the flow of RunCases for one target on top
of them: tissue run, then the water run on the same live engine. PhaseMap is np.angle of the fetched p_complex and stays with the caller, as do
DomeType domains and the refocusing flow. There is no CPU fallback."""
import ctypes as C
import operator

import numpy as np

from . import Domain as D
from . import _engine, _step1, harness, results
from .sources import SeparableSource

NAMES = {'p_amp': 0, 'p_complex': 1, 'peak': 2, 'MaterialMap': 3, 'MaterialMapNoCT': 4, 'AirMask': 5, 'map': 6, 'mapNoCT': 7, 'airOut': 8}
SLOTS = {'tissue': 0, 'water': 1, 'refocus': 2}
_DTYPES = {0: np.float32, 1: np.complex64, 2: np.float32, 3: np.uint32, 4: np.uint32, 5: np.uint8, 6: np.uint32, 7: np.uint32, 8: np.uint32}


class AcousticStudy:
    """The volumes of one acoustic calculation on one device. labels: uint8, as stored; ct_index: the index map of *CT.nii.gz (uint16 or uint32) or
    None; air: the mask of *AirRegions.nii.gz or None (read with a CT only, as in the reference). The host arrays are read once, here."""

    def __init__(self, labels, ct_index=None, air=None, device=None):
        self._h = None
        self.sim = None
        a = D._volume(labels, np.uint8, 'labels')
        ct = None if ct_index is None else D._ct_volume(ct_index, a.shape)
        ar = None if air is None or ct is None else D._volume(_step1.bool_as_uint8(np.asarray(air)), np.uint8, 'air', a.shape)
        self.labels, self.has_ct, self.has_air = a, ct is not None, ar is not None
        self.device = D._device if device is None else int(device)
        self.plan_, self.water_only = None, False
        self._shape = {}                      # output shape of each packed slot
        self._held = {}                       # (MaterialMapNoCT, AirMask) exist in each packed slot
        self._handed = 0                      # bytes of the tables and lists this study has handed to its engine's setters
        lib = self._lib = _engine.load_library()
        h = C.c_void_p()
        self._check(lib.bfd_acoustic_create(self.device, a.shape[0], a.shape[1], a.shape[2], 0 if ct is None else ct.itemsize, int(ar is not None), C.byref(h)),
                    'bfd_acoustic_create')
        self._h = h
        try:
            self._check(lib.bfd_acoustic_set_volumes(h, _engine._ptr(a), _engine._ptr(ct), _engine._ptr(ar)), 'bfd_acoustic_set_volumes')
        except Exception:
            self.close()
            raise

    # ---------------------------------------------------------------- lifetime ----------------------------------------------------------------
    def close(self):
        if self.sim is not None:
            self.sim.close()
            self.sim = None
        if self._h is not None:
            self._lib.bfd_acoustic_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()

    def _check(self, rc, entry):
        if rc != 0:
            raise _engine.EngineError('%s failed (rc=%d): %s' % (entry, rc, self._lib.bfd_last_error().decode()))

    def _handle(self):
        if self._h is None:
            raise _engine.EngineError('the acoustic study is closed')
        return self._h

    # ---------------------------------------------------------------- the domain ----------------------------------------------------------------
    def survey(self, labels=None, box=None, flip_k=True):
        """Domain.survey on the resident labels (its signature: plan_domain calls it; `labels` is not read)."""
        lo, hi = D._box(box, self.labels.shape)
        hist, bounds, focal = np.zeros(256, np.int64), np.zeros(6, np.int64), np.zeros(2, np.int64)
        P = _engine._ptr
        self._check(self._lib.bfd_acoustic_survey(self._handle(), P(lo), P(hi), int(bool(flip_k)), P(hist), P(bounds), P(focal)), 'bfd_acoustic_survey')
        return hist, bounds, focal

    def plan(self, SpatialStep, **kw):
        """Domain.plan_domain(labels, SpatialStep, **kw) with both surveys on the resident labels"""
        return D.plan_domain(self.labels, SpatialStep, survey=self.survey, **kw)

    def assemble(self, plan, n_materials=None, water_only=False, ct_offset=None):
        """Domain.assemble on the resident volumes; the maps stay on the device (fetch('map'), 'mapNoCT', 'airOut' bring them). Returns the stats
        dict (None with water_only: the map is zeros, formed on the device)."""
        D._check_plan(plan, self.labels.shape)
        if n_materials is not None:
            n_materials = operator.index(n_materials)
            if not 0 <= n_materials < 2 ** 32:
                raise ValueError('n_materials must be 0 .. 2^32 - 1, not %r' % (n_materials,))
        lo, hi = D._box((plan.box_lo, plan.box_hi), self.labels.shape)
        flip = bool(plan.flip_k)
        segmented, offset = False, 0
        if not water_only:
            segmented = bool(self.survey(None, (lo, hi), flip)[0][6:].any())                      # :2162, on the crop
            if self.has_ct:
                offset = operator.index(ct_offset) if ct_offset is not None else (6 if self.survey(None, None, flip)[0][6:].any() else 3)     # :1163
                if not 0 <= offset < 2 ** 32:
                    raise ValueError('ct_offset must be 0 .. 2^32 - 1, not %r' % (ct_offset,))
        lut = D.relabel_lut(self.has_ct, segmented)
        size = hi - lo
        padLo, padHi = np.array(plan.pad_lo, np.int64), np.array(plan.pad_hi, np.int64)
        if tuple(size + padLo + padHi) != tuple(plan.shape):
            raise ValueError('the plan is not consistent: box %r, offsets %r and %r, domain %r' % (tuple(size), plan.pad_lo, plan.pad_hi, plan.shape))
        focalIJ = np.array(plan.FocalSpotLocation[:2], np.int64)
        stats = np.zeros(8, np.int64)
        P = _engine._ptr
        self._check(self._lib.bfd_acoustic_assemble(self._handle(), P(lo), P(size), P(padLo), P(padHi), int(flip), P(lut), offset, int(plan.ZSourceLocation),
                                                    2 ** 32 - 1 if n_materials is None else n_materials, P(focalIJ), int(bool(water_only)), P(stats)),
                    'bfd_acoustic_assemble')
        self.plan_, self.water_only = plan, bool(water_only)
        if water_only:
            return None
        st = dict(zip(D.STATS, (int(x) for x in stats)))
        if self.has_ct:
            if st['bone_voxels'] == 0:
                raise ValueError('the crop holds no bone (labels 2, 3): SubCTMap[BoneRegion].min() of an empty array (:2191)')
            if not st['ct_min'] >= 3:
                raise ValueError('SubCTMap[BoneRegion].min()>=3 does not hold: the minimum is %d (:2191)' % st['ct_min'])
            if n_materials is not None and not st['ct_max'] <= n_materials:
                raise ValueError('SubCTMap[BoneRegion].max()<=self.ReturnArrayMaterial().shape[0] does not hold: the maximum is %d, the rows %d (:2192)'
                                 % (st['ct_max'], n_materials))
        return st

    # ---------------------------------------------------------------- the solver ----------------------------------------------------------------
    def _planned(self):
        if self.plan_ is None:
            raise _engine.EngineError('assemble comes first')
        return self.plan_

    def attach(self):
        """The resident map (and air mask) into the live engine: bfd_set_material_map_device / bfd_set_reflector_device"""
        self._check(self._lib.bfd_acoustic_attach(self._handle(), self.sim.h), 'bfd_acoustic_attach')

    def engine(self, MaterialList, Frequency, SpatialStep, dt, nt, QCorrection=1.0, sensorSub=1, sensorStart=0, reflectionLimit=1e-5, rmsFirstStep=0):
        """The Engine of this study's domain: Pressure RMS, the Pressure sensors of harness.sensor_maps's box set through bfd_set_sensor_box and
        accumulated in the loop (sensorMode 1), the resident map attached. Returns it; the study owns it."""
        plan = self._planned()
        if self.sim is not None:
            self.sim.close()
            self.sim = None
        ml = np.ascontiguousarray(MaterialList, np.float64).reshape(-1, 5)
        N1, N2, N3 = plan.shape
        pml, zsrc = plan.PMLThickness, int(plan.ZSourceLocation)
        self.sim = _engine.Engine(N1, N2, N3, ml.shape[0], SpatialStep, dt, Frequency, nt, NDelta=pml, reflectionLimit=reflectionLimit, sensorSub=sensorSub,
                                  sensorStart=sensorStart, selRMSorPeak=1, selMapsRMS=['Pressure'], selMapsSensors=['Pressure'], device=self.device,
                                  rmsFirstStep=rmsFirstStep, sensorMode=1)
        self.Frequency, self.dt, self.nt, self.rho_c = Frequency, dt, nt, ml[0, 0] * ml[0, 1]
        self.sim.set_materials(ml, QCorrection)
        self._handed += ml.nbytes + 8 * ml.shape[0]
        self.attach()
        self.sim.set_sensor_box((pml, pml, zsrc + 1), (N1 - 2 * pml, N2 - 2 * pml, N3 - pml - zsrc - 1))
        return self.sim

    def set_source_plane(self, u0, T=None, ramp_length=4):
        """The complex particle-velocity plane u0 (N1, N2) at ZSourceLocation as the CW sources of harness.cw_pulse_sources (rows in np.where order of
        the plane, weights Ox = Oy = 0, Oz = 1 / (rho0 c0), BASE:2325-2335): the lists come from the plane alone, no SourceMap volume is formed."""
        plan = self._planned()
        N1, N2, _ = plan.shape
        u0 = np.asarray(u0)
        if u0.shape != (N1, N2):
            raise ValueError('the source plane has shape %r, the domain %r' % (u0.shape, (N1, N2)))
        T = self.nt * self.dt if T is None else T
        ii, jj = np.where(np.abs(u0) > 0)
        src = SeparableSource.cw(u0[ii, jj], self.Frequency, self.dt, T, ramp_length)
        lin = ii.astype(np.int64) + N1 * (jj.astype(np.int64) + N2 * int(plan.ZSourceLocation))
        order = np.argsort(lin, kind='stable')
        n = len(lin)
        w = [np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, 1.0 / self.rho_c, np.float32)]
        self.sim.set_sources(lin[order], np.arange(n, dtype=np.int64)[order], w[0], w[1], w[2], src)
        self._handed += 4 * n * 5 + src.weights.nbytes + src.signals.nbytes
        return n

    def run(self, nSteps=None):
        self.sim.run(self.nt if nSteps is None else nSteps)
        self.sim.sync()

    def reset(self):
        self.sim.reset()

    # ---------------------------------------------------------------- results ----------------------------------------------------------------
    def pack(self, correction=None, slot=0, full=False, flipK=True):
        """The results of the run into the resident volumes of `slot` (0 / 'tissue', 1 / 'water', 2 / 'refocus'): scattered, scaled by the
        dispersion correction (None: not at all), zeroed up to the source plane, cropped to the plan's kept region and flipped; the maps with them.
        full: pasted into a volume of the mask's shape at the shrinks (paste_and_flip) instead of the kept size (DataForSim)."""
        plan = self._planned()
        crop = plan.crop()
        kept = [n - l - h for n, l, h in zip(plan.shape, crop.lo, crop.hi)]
        O, at = (list(plan.mask_shape), list(crop.shrink)) if full else (kept, [0, 0, 0])
        sp = _engine.pack_spec(crop.lo, crop.hi, plan.ZSourceLocation, O, at, flipK, correction)
        slot = SLOTS.get(slot, slot)
        self._check(self._lib.bfd_acoustic_pack(self._handle(), self.sim.h, C.byref(sp), int(slot)), 'bfd_acoustic_pack')
        self._shape[slot] = tuple(O)
        self._held[slot] = (self.has_ct and not self.water_only, self.has_air and not self.water_only)      # what the slot's maps are, as the handle records it

    def fetch(self, name, slot=0):
        """One volume to the host: 'p_amp', 'p_complex', 'peak', 'MaterialMap' (the map the engine ran on), 'MaterialMapNoCT', 'AirMask' of a packed
        slot, or the whole assembled 'map', 'mapNoCT', 'airOut'."""
        which = NAMES[name]
        slot = SLOTS.get(slot, slot)
        shape = self._planned().shape if which >= 6 else self._shape.get(slot, (0, 0, 0))
        out = np.zeros(shape, _DTYPES[which])
        self._check(self._lib.bfd_acoustic_get(self._handle(), which, int(slot), _engine._ptr(out)), 'bfd_acoustic_get')
        return out

    def data_for_sim(self, Material, zLengthBeyonFocalPoint, slot=0):
        """The dict of results.data_for_sim for a slot packed at the kept size: the volumes fetched, the small entries formed here."""
        plan = self._planned()
        crop = plan.crop()
        with_ct, with_air = self._held.get(SLOTS.get(slot, slot), (self.has_ct, self.has_air))
        d = {'p_amp': self.fetch('p_amp', slot), 'p_complex': self.fetch('p_complex', slot)}
        if with_ct:
            d['MaterialMapCT'] = self.fetch('MaterialMap', slot)
            d['MaterialMap'] = self.fetch('MaterialMapNoCT', slot)
        else:
            d['MaterialMap'] = self.fetch('MaterialMap', slot)
        if with_air:
            d['AirMask'] = self.fetch('AirMask', slot)
        f = np.asarray(plan.FocalSpotLocation, int) - np.array(crop.lo)
        if np.any(f < 0) or np.any(f >= np.array(d['MaterialMap'].shape)):
            raise ValueError('the focal spot lies outside the kept region')
        d['Material'] = np.asarray(Material)
        (x0, y0, z0), (x1, y1, z1) = crop.lo, crop.hi
        d['x_vec'], d['y_vec'], d['z_vec'] = np.asarray(plan.XDim)[x0:-x1], np.asarray(plan.YDim)[y0:-y1], np.asarray(plan.ZDim)[z0:-z1]
        d['SpatialStep'] = plan.SpatialStep
        d['TargetLocation'] = f.astype(np.int64)
        d['zLengthBeyonFocalPoint'] = zLengthBeyonFocalPoint
        return d

    def traffic(self):
        """(up, down) bytes between host and device on this study's account: what the handle copied (bfd_acoustic_traffic: the volumes once, the
        small words of each stage, every fetch) plus the material table and the source lists the study handed to its engine's setters."""
        up, down = C.c_int64(), C.c_int64()
        self._check(self._lib.bfd_acoustic_traffic(self._handle(), C.byref(up), C.byref(down)), 'bfd_acoustic_traffic')
        return up.value + self._handed, down.value


def acoustic_field(labels, MaterialList, Frequency, SpatialStep, source_plane, plan_kwargs, ct_index=None, air=None, QCorrection=1.0, steps=None,
                   zLengthBeyonFocalPoint=4e-2, device=None, water=True):
    """The flow of RunCases for one target on one device: plan, assemble, the tissue run and its DataForSim, then the map of water on the same live
    engine, a reset, the water run and its DataForSim. source_plane: callable(plan) -> the complex plane (N1, N2) at ZSourceLocation. steps: the
    number of time steps instead of the plan's own (tests). Returns dict(plan, stats, tissue, water, correction, traffic)."""
    ml = np.ascontiguousarray(MaterialList, np.float64).reshape(-1, 5)
    with AcousticStudy(labels, ct_index, air, device) as st:
        plan = st.plan(SpatialStep, **plan_kwargs)
        stats = st.assemble(plan, ml.shape[0])
        dt_ideal = _engine.stable_dt(ml, Frequency, True, SpatialStep, harness.ALPHA_CFL, QCorrection)
        dt_water = _engine.stable_dt(ml[:1], Frequency, True, SpatialStep, 1.0)
        ppp, dt = harness.ppp_rule(dt_ideal, Frequency)
        T, nt, sub, start = plan.time_plan(dt, ppp, ml[0, 1])
        if steps is not None:
            nt = int(steps)
            T = nt * dt
            start = max(int((nt - harness.CYCLES_TO_TRACK * ppp) / sub), 0)
        correction = harness.dispersion_correction(dt, dt_water)
        st.engine(ml, Frequency, SpatialStep, dt, nt, QCorrection, sensorSub=sub, sensorStart=start)
        st.set_source_plane(source_plane(plan), T)
        st.run()
        st.pack(correction, 'tissue')
        out = dict(plan=plan, stats=stats, correction=correction, dt=dt, nt=nt, tissue=st.data_for_sim(ml, zLengthBeyonFocalPoint, 'tissue'), water=None)
        if water:
            st.assemble(plan, ml.shape[0], water_only=True)
            st.attach()
            st.reset()
            st.run()
            st.pack(correction, 'water')
            out['water'] = st.data_for_sim(ml, zLengthBeyonFocalPoint, 'water')
        out['traffic'] = st.traffic()
    return out
