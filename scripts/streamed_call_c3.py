"""One whole drop-in call of C3 (512^3, 300 steps) with the dense source table streamed (BFD_SOURCE_TILE=64): wall time of the call and of its
prepare phase (classes, run lists, placement), the second call of the process. scripts/call_breakdown.py with bfd_prepare timed on its own."""
import os, sys, time, json
os.environ['BFD_SOURCE_TILE'] = '64'
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib
from babelbrain_amd import harness as H, _engine, RayleighAndBHTE
PMmod = importlib.import_module('babelbrain_amd.PropagationModel')

a, k, info = H.make_problem('C3', steps=300, stable_dt_fn=lambda ml, f, h, c: _engine.stable_dt(ml, f, True, h, c), forward=RayleighAndBHTE.ForwardSimple)
log = {}
E = _engine.Engine


class Spy(E):
    prepared = False

    def run(self, *aa, **kk):
        if not self.prepared:
            t = time.perf_counter(); self.prepare(); log['prepare'] = log.get('prepare', 0.0) + time.perf_counter() - t
            self.prepared = True
        t = time.perf_counter(); r = E.run(self, *aa, **kk); log['run'] = log.get('run', 0.0) + time.perf_counter() - t
        return r

    def set_sources(self, *aa, **kk):
        t = time.perf_counter(); r = E.set_sources(self, *aa, **kk); log['set_sources'] = log.get('set_sources', 0.0) + time.perf_counter() - t
        return r


PMmod.Engine = Spy
pm = PMmod.PropagationModel()
pm.StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)       # first call of the process: library load, code object upload
log.clear()
t0 = time.perf_counter(); out = pm.StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k); wall = time.perf_counter() - t0
res = {'lib': os.environ.get('BABELFDTD_HIP_LIB', 'branch'), 'call_s': round(wall, 4), 'prepare_s': round(log.get('prepare', -1), 4),
       'set_sources_s': round(log.get('set_sources', -1), 4), 'run_s': round(log.get('run', -1), 4), 'step_loop_s': round(pm.last_timing['total_ms'] / 1e3, 4),
       'peak': float(out[2]['Pressure'].max())}
print('CALL ' + json.dumps(res), flush=True)
