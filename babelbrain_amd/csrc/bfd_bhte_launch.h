// What the host side of the bio-heat solver (bfd_bhte.hip) needs of its kernels (bfd_bhte_kernels.hip): one typed launcher per thing a run queues. Each
// dispatches on the run's rev / idBytes to the kernel's instantiation and queues on the null stream. Host code only. Not part of the ABI.
#pragma once
#include "bfd_thermal_stages.h"
#include "bfd_bhte_plan_core.h"

// The widest material list (16-bit ids): the coefficient table the multi-step kernels keep in LDS (bfd_bhte_kernels.hip says how it is sized)
#define BFD_BHTE_MAX_MATERIALS 1536

// One pass of the plan from r.T[cur] to r.T[1 - cur]; g: the grid of a pass of p.length steps (unused for one step)
void bhte_launch_pass(const bfd_bhte_device_run &r, int cur, const bhte_pass &p, const bhte_geom &g);
// The monitors of the steps INSIDE pass p, recomputed from its input r.T[cur] (queued before the pass): the points by step_points / cone_points, a
// sample of the monitored plane by step_slice (first step) or cone_slice (steps in between)
void bhte_launch_inner_monitors(const bfd_bhte_device_run &r, int cur, const bhte_pass &p);
// The monitors of step s, read off its result r.T[cur]
void bhte_launch_monitors(const bfd_bhte_device_run &r, int cur, int s);
// The captures due at step boundary s, from capture nextCap on; returns the first capture that is not due yet
int bhte_launch_captures(const bfd_bhte_device_run &r, int cur, int s, int nextCap);
// Over n voxels: out = tab[mat]; q = (p p) qf[mat], where q may be p
void bhte_launch_table_lookup(int idBytes, const void *mat, const float *tab, float *out, size_t n);
void bhte_launch_heat_source(int idBytes, const float *p, const void *mat, const float *qf, float *q, size_t n);
