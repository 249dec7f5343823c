"""ctypes binding of libbabelfdtd_hip.so (include/babelfdtd.h): the solver classes and the host-side helpers. The signatures of
the entries, the structs and the loader are in _abi.py.

This is the thin layer BASELINE.json's north_star asks for: the reference's Python driver
(TranscranialModeling/BabelIntegrationBASE.py:2338) reaches the HIP engine through it.
There is no CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import ABI_SYMBOLS, ABI_VERSION, LIB_PATH, Config, EngineError, PackSpec  # noqa: F401 (the names callers import from here)
from .sources import SeparableSource

MAP_BITS = {'Vx': 0, 'Vy': 1, 'Vz': 2, 'Sigmaxx': 3, 'Sigmayy': 4, 'Sigmazz': 5,
            'Sigmaxy': 6, 'Sigmaxz': 7, 'Sigmayz': 8, 'Pressure': 9, 'ALLV': 10}
KIND_RMS, KIND_PEAK, KIND_LAST = 0, 1, 2
HALO_VELOCITY, HALO_STRESS = 0, 1
KERNEL_CLASSES = ['stress_fluid', 'stress_normal_solid', 'stress_shear_sparse', 'velocity_fluid', 'velocity_solid', 'fused_fluid']
FIELD_NAMES = ['Vx', 'Vy', 'Vz', 'Sxx', 'Syy', 'Szz', 'Sxy', 'Sxz', 'Syz', 'Rxx', 'Ryy', 'Rzz', 'Rxy', 'Rxz', 'Ryz']


def pack_spec(lo, hi, zSource, O, at=(0, 0, 0), flipK=True, correction=None):
    """The PackSpec of a kept region and an output: the one place where the two scales are formed. correction None: no scaling at all; else
    ampScale = correction * sqrt(2) in float64 (BASE:2440) and the factor itself."""
    i3 = C.c_int32 * 3
    scaled = correction is not None
    return PackSpec(i3(*[int(v) for v in lo]), i3(*[int(v) for v in hi]), int(zSource), i3(*[int(v) for v in O]), i3(*[int(v) for v in at]), int(bool(flipK)),
                    int(scaled), float(correction * np.sqrt(2)) if scaled else 0.0, float(correction) if scaled else 0.0)


_lib = None


def load_library():
    """The library at LIB_PATH, loaded once per process (_abi.load_library)."""
    global _lib
    if _lib is None:
        _lib = _abi.load_library(LIB_PATH)
    return _lib


def _check(rc, what):
    if rc != 0:
        raise EngineError('%s failed (rc=%d): %s' % (what, rc, load_library().bfd_last_error().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _estrides(a):
    return [s // a.itemsize for s in a.strides]


def mask_of(names):
    m = 0
    for n in names:
        if n not in MAP_BITS:
            raise ValueError('unknown map name %r (valid: %s)' % (n, ', '.join(MAP_BITS)))
        m |= 1 << MAP_BITS[n]
    return m


def ordered(names):
    return sorted(set(names), key=lambda n: MAP_BITS[n])


def list_devices():
    """[(ordinal, name)] -- counterpart of <backend>.ListDevices (SelFiles/SelFiles.py:245-262)."""
    lib = load_library()
    out = []
    for d in range(lib.bfd_device_count()):
        buf = C.create_string_buffer(256)
        _check(lib.bfd_device_name(d, buf, 256), 'bfd_device_name')
        out.append((d, buf.value.decode()))
    return out


def stable_dt(MaterialList, Frequency, QfactorCorrection, SpatialStep, AlphaCFL, QCorrection=1.0):
    lib = load_library()
    ml = np.ascontiguousarray(MaterialList, np.float64).reshape(-1, 5)
    qc = np.ascontiguousarray(np.broadcast_to(np.asarray(QCorrection, np.float64), (ml.shape[0],)))
    dt = lib.bfd_stable_dt(ml.shape[0], _ptr(ml), _ptr(qc), float(Frequency), int(bool(QfactorCorrection)),
                           float(SpatialStep), float(AlphaCFL))
    if dt <= 0:
        raise EngineError('bfd_stable_dt failed: ' + lib.bfd_last_error().decode())
    return dt


def material_tables(MaterialList, Frequency, QfactorCorrection, SpatialStep, dt, QCorrection=1.0):
    lib = load_library()
    ml = np.ascontiguousarray(MaterialList, np.float64).reshape(-1, 5)
    qc = np.ascontiguousarray(np.broadcast_to(np.asarray(QCorrection, np.float64), (ml.shape[0],)))
    t = np.zeros((7, ml.shape[0]), np.float32)
    c1k2 = np.zeros(2, np.float32)
    cmax = C.c_double()
    _check(lib.bfd_material_tables(ml.shape[0], _ptr(ml), _ptr(qc), float(Frequency), int(bool(QfactorCorrection)),
                                   float(SpatialStep), float(dt), _ptr(t), _ptr(c1k2), C.byref(cmax)),
           'bfd_material_tables')
    return t, c1k2, cmax.value


def dft_series(series, dt_sensor, freq, device=0):
    """Device single-bin DFT (+ peak) of a host (nSensor, nTs) float32 series: bfd_dft_series."""
    lib = load_library()
    x = np.ascontiguousarray(series, np.float32)
    F = np.zeros(x.shape[0], np.complex64)
    pk = np.zeros(x.shape[0], np.float32)
    _check(lib.bfd_dft_series(device, x.shape[0], x.shape[1], _ptr(x), float(dt_sensor), float(freq), _ptr(F.view(np.float32)), _ptr(pk)),
           'bfd_dft_series')
    return F, pk


class _Solver:
    """What Engine and Group share: the same calls under two entry prefixes (bfd_ for one engine, bfd_group_ for a group). The
    source index is local and uint32 for an engine, global and int64 for a group."""
    _prefix = None
    _index_type = None

    def _create(self, extra, selMapsRMS, selMapsSensors, qfactorCorrection, **cfg):
        """<prefix>create(cfg, *extra, &handle) with the bfd_config of the remaining keywords."""
        self.lib = load_library()
        if self.lib.bfd_device_count() <= 0:
            raise EngineError('no HIP device visible: the MI355X engine has no CPU fallback')
        self.selR = ordered(selMapsRMS)
        self.selS = ordered(selMapsSensors)
        self.cfg = Config(selMapsRMS=mask_of(self.selR), selMapsSensors=mask_of(self.selS), qfactorCorrection=int(bool(qfactorCorrection)), **cfg)
        self.h = C.c_void_p()
        _check(self._entry('create')(C.byref(self.cfg), *extra, C.byref(self.h)), self._prefix + 'create')
        self.shape = (cfg['N1'], cfg['N2'], cfg['nk'])

    def _entry(self, entry):
        return getattr(self.lib, self._prefix + entry)

    def _call(self, entry, *args):
        _check(self._entry(entry)(self.h, *args), self._prefix + entry)

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self._entry('destroy')(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs ----
    def set_materials(self, MaterialList, QCorrection=1.0):
        ml = np.ascontiguousarray(MaterialList, np.float64).reshape(-1, 5)
        if ml.shape[0] != self.cfg.nMat:
            raise ValueError('MaterialList rows != nMat')
        qc = np.ascontiguousarray(np.broadcast_to(np.asarray(QCorrection, np.float64), (ml.shape[0],)))
        self._call('set_materials', _ptr(ml), _ptr(qc))

    def _u32(self, a):
        a = np.asarray(a)
        assert a.shape == self.shape, (a.shape, self.shape)
        if a.dtype != np.uint32 or any(s < 0 for s in a.strides):
            a = np.ascontiguousarray(a, np.uint32)
        return a

    def set_reflector(self, mask):
        if mask is None:
            self._call('set_reflector', None, 0, 0, 0)
            return
        a = self._u32(mask)
        self._call('set_reflector', _ptr(a), *_estrides(a))

    def set_sources(self, index, row, wx, wy, wz, PulseSource):
        """PulseSource: the dense float64 [nSources][nT] table, or a SeparableSource (weights and signals stay resident)."""
        ix = np.asarray(index)
        if self._index_type is np.uint32 and ix.size and (int(ix.max()) >= 2 ** 32 or int(ix.min()) < 0):
            raise ValueError('source index beyond 2^32 voxels: split the domain over devices (devices=[...])')
        ix = np.ascontiguousarray(ix, self._index_type)
        rw = np.ascontiguousarray(row, np.uint32)
        ws = [None if w is None else np.ascontiguousarray(w, np.float32) for w in (wx, wy, wz)]
        if isinstance(PulseSource, SeparableSource):
            src = PulseSource
            self._call('set_sources_separable', ix.size, _ptr(ix), _ptr(rw), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]),
                       src.shape[0], src.K, _ptr(src.weights), src.shape[1], _ptr(src.signals))
            self._pulse = None      # only now: a streamed dense table set before is released by the call above
            return
        pulse = np.ascontiguousarray(np.atleast_2d(PulseSource), np.float64)
        self._pulse = pulse     # a large table is streamed from here in time tiles during the run: keep it alive with the solver
        self._call('set_sources', ix.size, _ptr(ix), _ptr(rw), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]), _ptr(pulse), pulse.shape[0], pulse.shape[1])

    def set_sensor_map(self, SensorMap):
        a = self._u32(SensorMap)
        n = C.c_int64()
        self._call('set_sensor_map', _ptr(a), *_estrides(a), C.byref(n))
        return n.value

    # ---- stepping ----
    def set_placement(self, mode=1, search_limit_bytes=-1):
        """Placement policy of the per-voxel arrays (bfd_set_placement), before the first step: mode 0 = off; search_limit_bytes =
        throw-away memory the search for another memory region may hold (< 0: default rule, nothing on a shared device)."""
        self._call('set_placement', int(mode), int(search_limit_bytes))

    def prepare(self):
        """Classes, run lists and the placement of the per-voxel arrays (bfd_prepare); before any halo() of a slab."""
        self._call('prepare')

    def run(self, nSteps):
        self._call('run', int(nSteps))

    def sync(self):
        self._call('sync')

    def reset(self):
        self._call('reset')

    # ---- outputs ----
    @property
    def num_sensors(self):
        return self._entry('num_sensors')(self.h)

    @property
    def num_sensor_steps(self):
        return self._entry('num_sensor_steps')(self.h)

    def sensor_index(self):
        idx = np.zeros(self.num_sensors, np.uint32)
        self._call('get_sensor_index', _ptr(idx))
        return idx

    def sensors(self):
        out = np.zeros((len(self.selS), self.num_sensors, max(self.num_sensor_steps, 0)), np.float32)
        self._call('get_sensors', _ptr(out))
        return out

    def sensor_dft(self, freq):
        """(F, peak): complex64 and float32 arrays [nSelSensors][nSensors] (bfd_get_sensor_dft)."""
        F = np.zeros((len(self.selS), self.num_sensors), np.complex64)
        pk = np.zeros((len(self.selS), self.num_sensors), np.float32)
        self._call('get_sensor_dft', float(freq), _ptr(F.view(np.float32)), _ptr(pk))
        return F, pk

    def get_map(self, kind, name, out=None):
        if out is None:
            out = np.zeros(self.shape, np.float32)
        self._call('get_map', kind, MAP_BITS[name], _ptr(out), *_estrides(out))
        return out

    @property
    def device_bytes(self):
        return self._entry('device_bytes')(self.h)


class Engine(_Solver):
    """One Z-slab of the domain on one GPU."""
    _prefix = 'bfd_'
    _index_type = np.uint32

    def __init__(self, N1, N2, N3, nMat, h, dt, freq, nt, k0=0, nk=None, NDelta=12, reflectionLimit=1e-5,
                 typeSource=0, sensorSub=1, sensorStart=0, selRMSorPeak=1, selMapsRMS=('Pressure',),
                 selMapsSensors=('Pressure',), qfactorCorrection=True, device=0, kernelVariant=0, rmsFirstStep=0, sensorMode=0):
        self._create((), selMapsRMS, selMapsSensors, qfactorCorrection, N1=N1, N2=N2, N3=N3, k0=k0, nk=N3 - k0 if nk is None else nk, nMat=nMat,
                     NDelta=NDelta, typeSource=typeSource, sensorSub=sensorSub, sensorStart=sensorStart, nt=nt, selRMSorPeak=selRMSorPeak, device=device,
                     kernelVariant=kernelVariant, rmsFirstStep=rmsFirstStep, sensorMode=sensorMode, h=h, dt=dt, freq=freq, reflectionLimit=reflectionLimit)

    # ---- inputs ----
    def set_stream(self, stream_ptr):
        self._call('set_stream', C.c_void_p(stream_ptr))

    def set_material_map(self, slab_with_ghosts, ghostLow, ghostHigh):
        """slab_with_ghosts: uint32 (N1,N2,ghostLow+nk+ghostHigh) view/array (any strides >= 0)."""
        a = np.asarray(slab_with_ghosts)
        if a.dtype != np.uint32:
            a = a.astype(np.uint32)
        assert a.shape == (self.shape[0], self.shape[1], self.shape[2] + ghostLow + ghostHigh), a.shape
        if any(s < 0 for s in a.strides):
            a = np.ascontiguousarray(a)
        s1, s2, s3 = _estrides(a)
        base = a.ctypes.data + ghostLow * a.strides[2]
        self._call('set_material_map', C.c_void_p(base), s1, s2, s3, ghostLow, ghostHigh)

    def _u32(self, a):
        a = super()._u32(a)
        # the ABI uploads the whole address span of the view: keep it dense
        if a.size and (sum((n - 1) * s for n, s in zip(a.shape, _estrides(a))) + 1) != a.size:
            a = np.ascontiguousarray(a)
        return a

    # ---- inputs that are on the device already ----
    def _device_view(self, t, shape):
        """(pointer, element strides) of a 4-byte integer torch tensor on this engine's device; what wrote it is waited for."""
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise TypeError('a torch tensor on the device is expected (host arrays go through the host setters)')
        if t.element_size() != 4 or t.is_floating_point():
            raise TypeError('a 32-bit integer tensor is expected, got %s' % t.dtype)
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
        if any(s < 0 for s in t.stride()):
            raise ValueError('negative strides are not supported')
        torch.cuda.current_stream(t.device).synchronize()       # the engine's stream waits for no other stream
        return t.data_ptr(), [int(s) for s in t.stride()]

    def set_material_map_device(self, slab_with_ghosts, ghostLow=0, ghostHigh=0):
        """set_material_map from a 32-bit integer torch tensor (N1,N2,ghostLow+nk+ghostHigh) on the engine's device, any strides >= 0:
        read in place (bfd_set_material_map_device). The tensor may be released when the call has returned."""
        p, st = self._device_view(slab_with_ghosts, (self.shape[0], self.shape[1], self.shape[2] + ghostLow + ghostHigh))
        self._call('set_material_map_device', C.c_void_p(p + 4 * ghostLow * st[2]), st[0], st[1], st[2], ghostLow, ghostHigh)

    def set_reflector_device(self, mask):
        """set_reflector from a 32-bit integer torch tensor of the slab's shape on the engine's device; None clears the mask."""
        if mask is None:
            self._call('set_reflector_device', None, 0, 0, 0)
            return
        p, st = self._device_view(mask, self.shape)
        self._call('set_reflector_device', C.c_void_p(p), *st)

    def set_sensor_box(self, lo, size):
        """The sensors of the dense box lo <= (i, j, k) < lo + size without a SensorMap volume (bfd_set_sensor_box); returns their number."""
        lo_, size_ = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(size, np.int32)
        assert lo_.shape == (3,) and size_.shape == (3,)
        n = C.c_int64()
        self._call('set_sensor_box', _ptr(lo_), _ptr(size_), C.byref(n))
        return n.value

    # ---- stepping ----
    def half_step_stress(self, part=0, stream=None):
        """stream: raw HIP stream handle (int) to launch this part on, without synchronisation; None = the engine's stream."""
        if stream is None:
            self._call('half_step_stress_part', part)
        else:
            self._call('half_step_stress_part_on', part, C.c_void_p(stream))

    def half_step_velocity(self, part=0, stream=None):
        if stream is None:
            self._call('half_step_velocity_part', part)
        else:
            self._call('half_step_velocity_part_on', part, C.c_void_p(stream))

    def halo_fields(self):
        """Which fields of each halo group this slab reads from its Z-neighbours' planes:
        an all-fluid slab (tiled kernels, no solid tile) needs only Vz and Szz."""
        out = {}
        for g in (HALO_VELOCITY, HALO_STRESS):
            m = C.c_uint32()
            self._call('halo_fields', g, C.byref(m))
            out[g] = [f for f in range(3) if m.value & (1 << f)]
        return out

    @property
    def step(self):
        return self.lib.bfd_current_step(self.h)

    def halo_region(self, group, f, side, send):
        p = C.c_void_p()
        n = C.c_size_t()
        self._call('halo_region', group, f, side, int(send), C.byref(p), C.byref(n))
        return p.value, n.value

    def timing_begin(self, perKernel=False):
        """perKernel: False/0 whole window only, True/1 + per half-step, 2 + per kernel class (timing_kernels)."""
        self._call('timing_begin', int(perKernel))

    def timing_end(self):
        d = [C.c_double() for _ in range(4)]
        n = [C.c_int64() for _ in range(2)]
        self._call('timing_end', *[C.byref(x) for x in d], *[C.byref(x) for x in n])
        return {'total_ms': d[0].value, 'stress_ms': d[1].value, 'velocity_ms': d[2].value, 'other_ms': d[3].value,
                'n_stress': n[0].value, 'n_velocity': n[1].value}

    def timing_kernels(self):
        """After timing_begin(2) ... timing_end(): {class: (total ms, launches)} per kernel class."""
        ms = np.zeros(len(KERNEL_CLASSES), np.float64)
        n = np.zeros(len(KERNEL_CLASSES), np.int64)
        self._call('timing_kernels', _ptr(ms), _ptr(n))
        return {c: (float(ms[i]), int(n[i])) for i, c in enumerate(KERNEL_CLASSES)}

    def algorithmic_bytes(self, accumulating=True):
        """Algorithmic bytes per launch of each kernel class (bfd_algorithmic_bytes)."""
        b = np.zeros(len(KERNEL_CLASSES), np.float64)
        self._call('algorithmic_bytes', int(bool(accumulating)), _ptr(b))
        return {c: float(b[i]) for i, c in enumerate(KERNEL_CLASSES)}

    def paired_launches(self):
        """Launches of the pairing stress flavour so far (paired Pressure accumulation; 0 = every step accumulated in the velocity kernels)."""
        return int(self.lib.bfd_paired_launches(self.h)) if hasattr(self.lib, 'bfd_paired_launches') else 0

    def placement_note(self):
        """What bfd_prepare found about the memory regions of the arrays and did about it."""
        return self.lib.bfd_placement_note(self.h).decode()

    # ---- outputs ----
    def pack_results(self, lo, hi, zSource, O=None, at=(0, 0, 0), flipK=True, correction=None, want=('p_amp', 'p_complex', 'peak')):
        """The Pressure results of a sensorMode 1 run as the cropped, zeroed, scaled and flipped volumes the caller saves, formed on the device
        (bfd_pack_results). lo / hi: the Crop offsets of the kept region; O: output shape (default: the kept size), at: where the kept region lands
        in it; correction: the dispersion factor (None: no scaling at all, not even the sqrt(2) of the amplitude). Returns
        {'p_amp': float32, 'p_complex': complex64, 'peak': float32} for the names in `want`, and the kernel time in 'kernel_ms'."""
        kept = [n - int(l) - int(h) for n, l, h in zip(self.shape, lo, hi)]
        O = kept if O is None else [int(v) for v in O]
        sp = pack_spec(lo, hi, zSource, O, at, flipK, correction)
        shape = tuple(max(v, 0) for v in O)
        out = {}
        if 'p_amp' in want:
            out['p_amp'] = np.zeros(shape, np.float32)
        if 'p_complex' in want:
            out['p_complex'] = np.zeros(shape, np.complex64)
        if 'peak' in want:
            out['peak'] = np.zeros(shape, np.float32)
        ms = C.c_float()
        cplx = out['p_complex'].view(np.float32) if 'p_complex' in out else None
        self._call('pack_results', C.byref(sp), _ptr(out.get('p_amp')), _ptr(cplx), _ptr(out.get('peak')), C.byref(ms))
        out['kernel_ms'] = ms.value
        return out

    def get_field(self, name, out=None):
        if out is None:
            out = np.zeros(self.shape, np.float32)
        self._call('get_field', FIELD_NAMES.index(name), _ptr(out), *_estrides(out))
        return out

    def tile_counts(self):
        n = [C.c_int32() for _ in range(5)]
        self._call('tile_counts', *[C.byref(x) for x in n])
        lean = C.c_int32()
        self._call('tile_count_lean', C.byref(lean))
        fused = C.c_int32()
        self._call('tile_count_fused', C.byref(fused))
        return {'lossless_fluid': n[0].value, 'lossy_fluid': n[1].value, 'solid': n[2].value,
                'uniform_fluid': n[3].value, 'pml_fluid': n[4].value, 'lean_fluid': lean.value, 'fused_fluid': fused.value}

    def activity_counts(self):
        """(active, total) sub-tiles of the quiet-run map; (0, 0) when the engine works on every tile in every half-step."""
        a, t = C.c_int64(), C.c_int64()
        self._call('activity_counts', C.byref(a), C.byref(t))
        return a.value, t.value


class _SlabView(Engine):
    """Engine-shaped view of one slab of a Group (per-slab queries: tile counts, timing, raw fields). Owned by the group."""

    def __init__(self, lib, handle, cfg, shape, selR, selS):      # noqa: super().__init__ would create an engine
        self.lib, self.h, self.cfg, self.shape, self.selR, self.selS = lib, handle, cfg, shape, selR, selS

    def close(self):
        self.h = None

    def __del__(self):
        pass


PEER_PATHS = {0: 'same device (device copy)', 1: 'peer access both ways (direct hipMemcpyPeerAsync)', 2: 'STAGED through the host (peer access missing)'}


def decode_peer_status(codes, devices=None):
    """Status words of bfd_group_peer_status -> one dict per interface r | r+1: path, can_access / enabled in each direction."""
    out = []
    for r, c in enumerate(np.asarray(codes, np.int64).tolist()):
        e = {'interface': r, 'path': PEER_PATHS.get(c & 15, 'unknown'), 'direct': (c & 15) != 2,
             'can_access': [bool(c & 16), bool(c & 64)], 'enabled': [bool(c & 32), bool(c & 128)]}
        if devices is not None and r + 1 < len(devices):
            e['devices'] = [int(devices[r]), int(devices[r + 1])]
        out.append(e)
    return out


def placement_cache_release():
    """Frees the device buffers kept between solver calls for the placement of the arrays; returns the bytes freed."""
    return int(load_library().bfd_placement_cache_release())


class Group(_Solver):
    """One solver call split into Z-slabs over several HIP devices of this process (bfd_group_*): whole-domain inputs and
    outputs, step loop and halo copies inside the library."""
    _prefix = 'bfd_group_'
    _index_type = np.int64

    def __init__(self, devices, N1, N2, N3, nMat, h, dt, freq, nt, NDelta=12, reflectionLimit=1e-5, typeSource=0, sensorSub=1,
                 sensorStart=0, selRMSorPeak=1, selMapsRMS=('Pressure',), selMapsSensors=('Pressure',), qfactorCorrection=True,
                 kernelVariant=0, rmsFirstStep=0, sensorMode=0):
        self.devices = [int(d) for d in devices]
        dv = np.ascontiguousarray(self.devices, np.int32)
        self._create((len(self.devices), _ptr(dv)), selMapsRMS, selMapsSensors, qfactorCorrection, N1=N1, N2=N2, N3=N3, k0=0, nk=N3, nMat=nMat,
                     NDelta=NDelta, typeSource=typeSource, sensorSub=sensorSub, sensorStart=sensorStart, nt=nt, selRMSorPeak=selRMSorPeak,
                     device=self.devices[0], kernelVariant=kernelVariant, rmsFirstStep=rmsFirstStep, sensorMode=sensorMode, h=h, dt=dt, freq=freq,
                     reflectionLimit=reflectionLimit)

    @property
    def size(self):
        return self.lib.bfd_group_size(self.h)

    def slab(self, r):
        """(k0, nk, device, engine view) of slab r."""
        k0, nk, dev, sim = C.c_int32(), C.c_int32(), C.c_int32(), C.c_void_p()
        self._call('slab', r, C.byref(k0), C.byref(nk), C.byref(dev), C.byref(sim))
        cfg = Config.from_buffer_copy(self.cfg)
        cfg.k0, cfg.nk, cfg.device = k0.value, nk.value, dev.value
        return k0.value, nk.value, dev.value, _SlabView(self.lib, sim, cfg, (self.shape[0], self.shape[1], nk.value), self.selR, self.selS)

    def set_material_map(self, MaterialMap):
        a = self._u32(MaterialMap)
        self._call('set_material_map', _ptr(a), *_estrides(a))

    def timing_begin(self):
        self._call('timing_begin')

    def timing_end(self):
        d = [C.c_double() for _ in range(4)]
        ov = C.c_int32()
        self._call('timing_end', *[C.byref(x) for x in d], C.byref(ov))
        return {'total_ms': d[0].value, 'max_device_ms': d[1].value, 'host_issue_ms': d[2].value, 'halo_bytes_per_step': d[3].value,
                'overlapped': bool(ov.value), 'slabs': self.size, 'peer': self.peer_status()}

    def peer_status(self):
        """How the halo planes cross each interface (bfd_group_peer_status), decoded: one dict per interface."""
        n = max(self.size - 1, 0)
        codes = np.zeros(max(n, 1), np.int32)
        got = self.lib.bfd_group_peer_status(self.h, _ptr(codes), n)
        if got < 0:
            _check(got, 'bfd_group_peer_status')
        return decode_peer_status(codes[:n], self.devices)

