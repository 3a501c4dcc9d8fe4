/*
 * Stand-alone check of the COUNT(DISTINCT) regroup's shared functions
 * (greengage_amd/csrc/plan_distinct.h): compiled from that header alone, with
 * any host C++17 compiler and no HIP, plain and under the address and
 * undefined-behaviour sanitizers (tests/test_plan_distinct_cpu.py).  Every
 * expectation is written out by hand.  Prints "ok <checks>" and exits 0, or
 * names the first failing line and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../greengage_amd/csrc/plan_distinct.h"

using gg::PlanRegroupDev;
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

/* the packed code of (v0, v1); has = 0 makes the field NULL */
static long long
pack(const PlanRegroupDev &G, bool has0, long long v0, bool has1, long long v1)
{
	u64 e0 = has0 ? (u64) v0 - (u64) G.gp.gmin[0] + 1 : 0;
	u64 e1 = has1 ? (u64) v1 - (u64) G.gp.gmin[1] + 1 : 0;

	return (long long) ((e0 << G.gp.shift) | e1);
}

static PlanRegroupDev
packed(int shift, long long min0, long long min1)
{
	PlanRegroupDev G = {};

	G.gp.packed = 1;
	G.gp.shift = shift;
	G.gp.gmin[0] = min0;
	G.gp.gmin[1] = min1;
	G.ngroup = 2;
	G.naggs = 1;
	G.kind[0] = 1;
	G.dmask = 1;
	return G;
}

static void
check_code()
{
	/* packed pairs with negative minima, NULL in either field */
	PlanRegroupDev G = packed(12, -1000, -7);

	CHECK(gg::plan_regroup_code(G, pack(G, true, -1000, true, -7)) == -1000);
	CHECK(gg::plan_regroup_code(G, pack(G, true, -1, true, 4000)) == -1);
	CHECK(gg::plan_regroup_code(G, pack(G, true, 123456, false, 0))
	      == 123456);
	CHECK(gg::plan_regroup_code(G, pack(G, false, 0, true, 5)) == NULLK);
	CHECK(gg::plan_regroup_code(G, pack(G, false, 0, false, 0)) == NULLK);
	CHECK(gg::plan_regroup_code(G, 0) == NULLK);
	/* by hand: e0 = 3, e1 = 9 */
	CHECK(gg::plan_regroup_code(G, (3ll << 12) | 9) == -998);

	/* shift 1: the distinct column is empty or all NULL (e1 is 0 or 1) */
	G = packed(1, -5, 0);
	CHECK(gg::plan_regroup_code(G, pack(G, true, -5, true, 0)) == -5);
	CHECK(gg::plan_regroup_code(G, pack(G, true, 7, false, 0)) == 7);
	CHECK(gg::plan_regroup_code(G, (13ll << 1) | 1) == 7);
	CHECK(gg::plan_regroup_code(G, 1) == NULLK);

	/* shift 61: a one-bit group column beside a 61-bit distinct one */
	G = packed(61, -3, -(1ll << 59));
	CHECK(gg::plan_regroup_code(G, pack(G, true, -3, true, (1ll << 59)))
	      == -3);
	CHECK(gg::plan_regroup_code(G, (1ll << 61) | ((1ll << 61) - 1)) == -3);
	CHECK(gg::plan_regroup_code(G, pack(G, false, 0, true, -(1ll << 59)))
	      == NULLK);
	CHECK(gg::plan_regroup_code(G, (1ll << 61) - 1) == NULLK);

	/* two char1 columns: e0 * 512 + e1, 256 = NULL */
	PlanRegroupDev C = {};

	C.ngroup = 2;
	C.naggs = 1;
	CHECK(gg::plan_regroup_code(C, 65 * 512 + 66) == 65);
	CHECK(gg::plan_regroup_code(C, 255 * 512 + 256) == 255);
	CHECK(gg::plan_regroup_code(C, 0 * 512 + 255) == 0);
	CHECK(gg::plan_regroup_code(C, 256 * 512 + 7) == NULLK);
	CHECK(gg::plan_regroup_code(C, 256 * 512 + 256) == NULLK);

	/* inner ngroup == 1: no outer group column, every code is 0 */
	PlanRegroupDev S = {};

	S.ngroup = 1;
	S.naggs = 1;
	CHECK(gg::plan_regroup_code(S, 0) == 0);
	CHECK(gg::plan_regroup_code(S, -123456789) == 0);
	CHECK(gg::plan_regroup_code(S, NULLK) == 0);
	CHECK(gg::plan_regroup_code(S, 0x7fffffffffffffffll) == 0);
}

/* slots: 0 COUNT(*), 1 distinct COUNT(x), 2 SUM, 3 MIN word, 4 MAX word,
 * 5 helper count */
static PlanRegroupDev
six_slots(const PlanRegroupDev &base)
{
	PlanRegroupDev G = base;

	G.naggs = 6;
	G.kind[0] = 0;
	G.kind[1] = 1;
	G.kind[2] = 2;
	G.kind[3] = 3;
	G.kind[4] = 4;
	G.kind[5] = 1;
	G.dmask = 1u << 1;
	return G;
}

static void
check_contrib()
{
	PlanRegroupDev G = six_slots(packed(8, 0, 0));
	u64 lo = 99, hi = 99;

	/* kinds 0..2: the 128-bit value, zero contributing nothing */
	CHECK(gg::plan_regroup_contrib(G, 0, 5, 0, &lo, &hi) && lo == 5 &&
	      hi == 0);
	CHECK(!gg::plan_regroup_contrib(G, 0, 0, 0, &lo, &hi));
	CHECK(gg::plan_regroup_contrib(G, 5, 3, 0, &lo, &hi) && lo == 3 &&
	      hi == 0);
	/* a negative SUM partial: -5 as two words */
	CHECK(gg::plan_regroup_contrib(G, 2, ~0ull - 4, ~0ull, &lo, &hi) &&
	      lo == ~0ull - 4 && hi == ~0ull);
	CHECK(gg::plan_regroup_contrib(G, 2, 0, 1, &lo, &hi) && lo == 0 &&
	      hi == 1);
	/* MIN / MAX words: word 0 alone, 0 = no input */
	CHECK(gg::plan_regroup_contrib(G, 3, 0x8000000000000005ull, 0, &lo, &hi)
	      && lo == 0x8000000000000005ull && hi == 0);
	CHECK(!gg::plan_regroup_contrib(G, 3, 0, 0, &lo, &hi));
	CHECK(!gg::plan_regroup_contrib(G, 4, 0, 7, &lo, &hi));
	CHECK(gg::plan_regroup_contrib(G, 4, 1, 7, &lo, &hi) && lo == 1 &&
	      hi == 0);
	/* a distinct slot: 1 however many rows carried the value */
	CHECK(gg::plan_regroup_contrib(G, 1, 1, 0, &lo, &hi) && lo == 1 &&
	      hi == 0);
	CHECK(gg::plan_regroup_contrib(G, 1, 4000000000ull, 0, &lo, &hi) &&
	      lo == 1 && hi == 0);
	CHECK(gg::plan_regroup_contrib(G, 1, 0, 2, &lo, &hi) && lo == 1 &&
	      hi == 0);
	CHECK(!gg::plan_regroup_contrib(G, 1, 0, 0, &lo, &hi));
}

static void
check_rows()
{
	PlanRegroupDev G = six_slots(packed(8, -10, 100));
	const u64 MSB = 0x8000000000000000ull;
	std::vector<u64> in, out;
	auto row = [&](long long code, std::vector<u64> words)
	{
		in.push_back((u64) code);
		in.insert(in.end(), words.begin(), words.end());
	};

	/* group 5: three values, one of them with no counted row, and a
	 * NULL-value pair; the SUM partials carry out of the low word and one
	 * is negative; MIN / MAX words with a "no input" 0 among them */
	row(pack(G, true, 5, true, 100),
	    {2, 0, 2, 0, ~0ull, 0, MSB | 9, 0, MSB | 3, 0, 2, 0});
	row(pack(G, true, 5, true, 101),
	    {1, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0});
	row(pack(G, true, 5, true, 300),
	    {4, 0, 4, 0, ~0ull - 1, ~0ull, MSB | 2, 0, MSB | 8, 0, 4, 0});
	row(pack(G, true, 5, false, 0),
	    {7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
	/* the NULL group: one value */
	row(pack(G, false, 0, true, 100),
	    {1, 0, 1, 0, 6, 0, MSB | 1, 0, MSB | 1, 0, 1, 0});
	/* group -10: NULL values only, so it exists with count 0 */
	row(pack(G, true, -10, false, 0),
	    {3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
	gg::plan_regroup_rows(G, in, &out);

	/* ordered by outer code: NULL_KEY, -10, 5.  Group 5's SUM is
	 * (2^64 - 1) + 3 + (-2): lo = 0, hi = 1 */
	const std::vector<u64> exp = {
		(u64) NULLK, 1, 0, 1, 0, 6, 0, MSB | 1, 0, MSB | 1, 0, 1, 0,
		(u64) -10ll, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
		5, 14, 0, 2, 0, 0, 1, MSB | 9, 0, MSB | 8, 0, 6, 0};

	CHECK(out.size() == exp.size());
	CHECK(out == exp);

	/* a SUM that goes negative across the fold: 1 + (-3) */
	in.clear();
	row(pack(G, true, 0, true, 100), {1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0});
	row(pack(G, true, 0, true, 101),
	    {1, 0, 1, 0, ~0ull - 2, ~0ull, 0, 0, 0, 0, 0, 0});
	gg::plan_regroup_rows(G, in, &out);
	CHECK((out == std::vector<u64>{0, 2, 0, 2, 0, ~0ull - 1, ~0ull, 0, 0, 0,
				       0, 0, 0}));

	/* no outer group column: everything folds into code 0, whatever the
	 * inner code, and a distinct slot with lo == 0, hi != 0 counts */
	PlanRegroupDev S = six_slots(PlanRegroupDev{});

	S.ngroup = 1;
	in.clear();
	row(-77, {1, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0});
	row(NULLK, {2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
	row(12, {3, 0, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0});
	gg::plan_regroup_rows(S, in, &out);
	CHECK((out == std::vector<u64>{0, 6, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0}));

	/* zero rows give zero rows, also without a group column: the
	 * executor supplies that plan's single empty row */
	in.clear();
	gg::plan_regroup_rows(S, in, &out);
	CHECK(out.empty());
	gg::plan_regroup_rows(G, in, &out);
	CHECK(out.empty());
}

int
main()
{
	check_code();
	check_contrib();
	check_rows();
	std::printf("ok %d\n", checks);
	return 0;
}
