/*
 * Stand-alone driver for the HAVING row test of compiled plans
 * (greengage_amd/csrc/plan_having.h), built and run by
 * test_plan_having_cpu.py with a plain host compiler: the header needs no
 * HIP.  One query per input line, one answer per line:
 *   R nclauses natoms[0] .. natoms[nclauses-1]
 *     then per atom, clause by clause:
 *       kind val slot cnt lo_hi lo_lo hi_hi hi_lo
 *     then nwords and the nwords u64 words of one compacted row
 *   -> 0 | 1 (plan_having_row), or E for a query that does not parse or
 *      names a word outside the row
 * kind is a gg_plan_havingkind, val a gg::PlanHavingVal; the _hi halves are
 * signed and the _lo halves and row words unsigned decimal numbers.
 */
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../greengage_amd/csrc/plan_having.h"

static bool query(std::istringstream &in, int *ans)
{
	gg::PlanHavingDev H = {};
	int total = 0, nwords = 0;

	if (!(in >> H.nclauses) || H.nclauses < 0 ||
	    H.nclauses > GG_PLAN_MAX_HAVING_CLAUSES)
		return false;
	for (int c = 0; c < H.nclauses; c++)
	{
		int n;

		if (!(in >> n) || n < 0 || n > GG_PLAN_MAX_HAVING_ATOMS)
			return false;
		H.natoms[c] = (int8_t) n;
		total += n;
	}
	if (total > GG_PLAN_MAX_HAVING_TOTAL)
		return false;
	for (int a = 0; a < total; a++)
	{
		gg::PlanHavingAtomDev &A = H.atoms[a];
		int kind, val, slot, cnt;

		if (!(in >> kind >> val >> slot >> cnt >> A.lo_hi >> A.lo_lo >>
		      A.hi_hi >> A.hi_lo))
			return false;
		if (slot < 0 || cnt < 0 || slot > 60 || cnt > 60)
			return false;
		A.kind = (int8_t) kind;
		A.val = (int8_t) val;
		A.slot = (int8_t) slot;
		A.cnt = (int8_t) cnt;
	}
	if (!(in >> nwords) || nwords < 1 || nwords > 200)
		return false;
	std::vector<unsigned long long> row(nwords);

	for (int w = 0; w < nwords; w++)
		if (!(in >> row[w]))
			return false;
	for (int a = 0; a < total; a++)
		if (2 + 2 * H.atoms[a].slot >= nwords ||
		    1 + 2 * H.atoms[a].cnt >= nwords)
			return false;
	*ans = gg::plan_having_row(H, row.data()) ? 1 : 0;
	return true;
}

int main()
{
	std::string line;

	while (std::getline(std::cin, line))
	{
		std::istringstream in(line);
		char cmd = 0;
		int ans = 0;

		if ((in >> cmd) && cmd == 'R' && query(in, &ans))
			std::cout << ans << "\n";
		else
			std::cout << "E\n";
	}
	return 0;
}
