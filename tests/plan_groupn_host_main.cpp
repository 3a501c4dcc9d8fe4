/*
 * Stand-alone check of the group-key decoder (greengage_amd/csrc/plan_keys.h)
 * for codes of three and four packed fields: compiled from that header alone,
 * with any host C++17 compiler and no HIP, plain and under the address and
 * undefined-behaviour sanitizers (tests/test_plan_groupn_cpu.py).  Codes are
 * packed here by hand, field by field, and must decode to the keys they were
 * made from; plan_code_of must give the same codes.  Prints "ok <checks>" and
 * exits 0, or names the first failing line and exits 1.
 */
#include <cstdio>
#include <cstdlib>

#include "../greengage_amd/csrc/plan_keys.h"

using gg::PlanGroupPackDev;
using gg::PlanKeysN;
typedef unsigned long long u64;

static int checks = 0;

#define CHECK(c) \
	do { \
		checks++; \
		if (!(c)) \
		{ \
			std::printf("FAILED line %d: %s\n", __LINE__, #c); \
			std::exit(1); \
		} \
	} while (0)

static const long long NULLK = GG_PLAN_NULL_KEY;

/* n fields of the given widths, field 0 most significant */
static PlanKeysN
fields(int n, const int *bits, const long long *mins)
{
	PlanKeysN N = {};
	int below = 0;

	N.n = n;
	for (int g = n - 1; g >= 0; g--)
	{
		N.shift[g] = below;
		N.gmin[g] = mins[g];
		below += bits[g];
	}
	return N;
}

/* the code by hand: e = 0 for NULL, else v - min + 1, concatenated */
static long long
pack(int n, const int *bits, const long long *mins, const long long *v,
     const bool *has)
{
	u64 code = 0;

	for (int g = 0; g < n; g++)
	{
		u64 e = has[g] ? (u64) v[g] - (u64) mins[g] + 1 : 0;

		code = (code << bits[g]) | e;
	}
	return (long long) code;
}

/* v round-trips through the code, by hand and by plan_code_of */
static void
roundtrip(int n, const int *bits, const long long *mins, const long long *v,
	  const bool *has)
{
	const PlanKeysN N = fields(n, bits, mins);
	const PlanGroupPackDev G = {};
	const long long code = pack(n, bits, mins, v, has);
	int64_t kin[PL_MAX_GCOLS] = {}, k[PL_MAX_GCOLS];
	int total = 0;

	for (int g = 0; g < n; g++)
	{
		kin[g] = v[g];
		total += bits[g];
	}
	CHECK(total <= 62);
	CHECK(code >= 0 && (u64) code < (1ull << 62));
	CHECK((u64) code != PL_EMPTY);
	CHECK(gg::plan_code_of(N, kin, has) == code);
	gg::plan_keys_of(G, N, n, code, k);
	for (int g = 0; g < n; g++)
		CHECK(k[g] == (has[g] ? v[g] : NULLK));
	for (int g = n; g < PL_MAX_GCOLS; g++)
		CHECK(k[g] == 0);
}

static void
check_shape(int n, const int *bits, const long long *mins)
{
	long long lo[PL_MAX_GCOLS] = {}, hi[PL_MAX_GCOLS] = {},
		mix[PL_MAX_GCOLS] = {};
	bool all[PL_MAX_GCOLS] = {true, true, true, true};

	for (int g = 0; g < n; g++)
	{
		/* 2^b - 1 values besides NULL: the last is min + 2^b - 2 */
		lo[g] = mins[g];
		hi[g] = (long long) ((u64) mins[g] + ((1ull << bits[g]) - 2));
		mix[g] = g & 1 ? hi[g] : lo[g];
	}
	/* every maximum together, every minimum together: no field carries
	 * into its neighbour */
	roundtrip(n, bits, mins, hi, all);
	roundtrip(n, bits, mins, lo, all);
	roundtrip(n, bits, mins, mix, all);
	/* NULL in each position, beside maxima and beside minima, and
	 * everywhere */
	for (int z = 0; z < n; z++)
	{
		bool has[PL_MAX_GCOLS] = {true, true, true, true};

		has[z] = false;
		roundtrip(n, bits, mins, hi, has);
		roundtrip(n, bits, mins, lo, has);
	}
	bool none[PL_MAX_GCOLS] = {false, false, false, false};

	roundtrip(n, bits, mins, lo, none);
}

/* distinct NULL positions give distinct codes, and the code orders as the
 * key tuple does with NULL first */
static void
check_order()
{
	const int bits[3] = {3, 4, 5};
	const long long mins[3] = {-2, 100, -(1ll << 40)};
	const long long a[3] = {-1, 105, -(1ll << 40) + 7};
	const bool n0[3] = {false, true, true}, n1[3] = {true, false, true},
		n2[3] = {true, true, false}, all[3] = {true, true, true};
	const long long c0 = pack(3, bits, mins, a, n0),
		c1 = pack(3, bits, mins, a, n1), c2 = pack(3, bits, mins, a, n2),
		ca = pack(3, bits, mins, a, all);

	CHECK(c0 != c1 && c1 != c2 && c0 != c2 && ca != c0 && ca != c1 &&
	      ca != c2);
	/* (NULL, ...) < (a0, NULL, ...) < (a0, a1, NULL) < (a0, a1, a2) */
	CHECK(c0 < c1 && c1 < c2 && c2 < ca);
	const long long b[3] = {-1, 106, -(1ll << 40)};

	CHECK(pack(3, bits, mins, b, all) > ca);
}

/* a plan with at most two columns decodes as it always did */
static void
check_two_column_plans()
{
	PlanGroupPackDev G = {};
	const PlanKeysN none = {};
	int64_t k[PL_MAX_GCOLS], k0, k1;

	G.packed = 1;
	G.shift = 12;
	G.gmin[0] = -1000;
	G.gmin[1] = -7;
	const long long code = (long long) ((5ull << 12) | 9ull);

	gg::plan_keys_of(G, 2, code, &k0, &k1);
	gg::plan_keys_of(G, none, 2, code, k);
	CHECK(k0 == -996 && k1 == 1 && k[0] == k0 && k[1] == k1);
	CHECK(k[2] == 0 && k[3] == 0);
	G = PlanGroupPackDev{};
	gg::plan_keys_of(G, none, 2, 65 * 512 + 256, k);
	CHECK(k[0] == 65 && k[1] == NULLK && k[2] == 0 && k[3] == 0);
	gg::plan_keys_of(G, none, 1, NULLK, k);
	CHECK(k[0] == NULLK && k[1] == 0);
	gg::plan_keys_of(G, none, 1, -12345, k);
	CHECK(k[0] == -12345 && k[1] == 0);
}

int
main()
{
	{
		/* char1 + int32 + int64 */
		const int bits[3] = {9, 20, 30};
		const long long mins[3] = {0, -40, 1ll << 50};

		check_shape(3, bits, mins);
	}
	{
		/* the whole budget, three fields and four; minima at the
		 * types' ends */
		const int b3[3] = {1, 31, 30};
		const long long m3[3] = {7, INT32_MIN, INT64_MAX - (1ll << 30)};
		const int b4[4] = {20, 1, 40, 1};
		const long long m4[4] = {-(1ll << 19), 0, INT64_MIN + 2, -1};

		check_shape(3, b3, m3);
		check_shape(4, b4, m4);
	}
	{
		/* one wide field beside one-bit fields (empty columns) */
		const int bits[4] = {1, 59, 1, 1};
		const long long mins[4] = {0, -(1ll << 58), 0, 0};

		check_shape(4, bits, mins);
	}
	{
		const int bits[4] = {16, 16, 15, 15};
		const long long mins[4] = {-32768, 1000000007, -5, 0};

		check_shape(4, bits, mins);
	}
	check_order();
	check_two_column_plans();
	std::printf("ok %d\n", checks);
	return 0;
}
