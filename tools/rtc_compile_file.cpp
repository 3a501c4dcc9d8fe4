/* Host-only: compile ONE generated plan program (a GG_PLAN_RTC_DUMP file,
 * split at the "==== nbake=N ====" separators first) with exactly the
 * hipRTC options plan_rtc.cpp uses and write the code object, for
 * llvm-objdump -d / llvm-readelf --notes.  Needs no GPU.
 * Build: hipcc -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
 *            tools/rtc_compile_file.cpp -o tools/rtc_compile_file
 *            -L/opt/rocm/lib -lhiprtc
 * Usage: rtc_compile_file PROGRAM.cu OUT.co */
#include <hip/hiprtc.h>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

int
main(int argc, char **argv)
{
	if (argc != 3)
		return 2;
	std::stringstream src;
	hiprtcProgram prog;
	const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};

	src << std::ifstream(argv[1]).rdbuf();
	if (hiprtcCreateProgram(&prog, src.str().c_str(), "gg_plan.cu", 0,
				nullptr, nullptr) != HIPRTC_SUCCESS)
		return 2;
	if (hiprtcCompileProgram(prog, 3, opts) != HIPRTC_SUCCESS)
	{
		size_t ls = 0;

		hiprtcGetProgramLogSize(prog, &ls);
		std::string log(ls, 0);
		hiprtcGetProgramLog(prog, &log[0]);
		fprintf(stderr, "%s\n", log.c_str());
		return 1;
	}
	size_t csz = 0;

	hiprtcGetCodeSize(prog, &csz);
	std::string code(csz, 0);
	hiprtcGetCode(prog, &code[0]);
	std::ofstream(argv[2], std::ios::binary).write(code.data(), csz);
	return 0;
}
