/*
 * The group keys a compiled plan's group code stands for.  ONE definition
 * for every side: plan.cpp decodes every arena row with it, the device top-k
 * (plan_topk.hip) decodes the order's key entries with it, and the
 * COUNT(DISTINCT) regroup (plan_distinct.h) takes the outer key out of an
 * inner code with it, so none of them can drift apart.
 *
 * Plain C++: builds with any C++17 compiler, with or without HIP.
 */
#ifndef GG_PLAN_KEYS_H
#define GG_PLAN_KEYS_H

#include <stdint.h>

#include "plan_dev.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_KEYS_HD __host__ __device__
#else
#define GG_KEYS_HD
#endif

namespace gg
{

/* a NULL key is GG_PLAN_NULL_KEY */
GG_KEYS_HD static inline void
plan_keys_of(const PlanGroupPackDev &G, int ngroup, long long code,
	     int64_t *k0, int64_t *k1)
{
	if (G.packed)
	{
		/* (e0 << shift) | e1; e = 0 is NULL, else the
		 * value's offset from the column minimum, plus 1 */
		uint64_t e0 = (uint64_t) code >> G.shift;
		uint64_t e1 = (uint64_t) code & ((1ull << G.shift) - 1);

		*k0 = e0 ? (int64_t) ((uint64_t) G.gmin[0] + e0 - 1)
			: GG_PLAN_NULL_KEY;
		*k1 = e1 ? (int64_t) ((uint64_t) G.gmin[1] + e1 - 1)
			: GG_PLAN_NULL_KEY;
	}
	else if (ngroup == 2)
	{
		long long e0 = code / 512, e1 = code % 512;

		*k0 = e0 == 256 ? GG_PLAN_NULL_KEY : e0;
		*k1 = e1 == 256 ? GG_PLAN_NULL_KEY : e1;
	}
	else
	{
		*k0 = code;
		*k1 = 0;
	}
}

}				/* namespace gg */

#endif /* GG_PLAN_KEYS_H */
