// ASan/UBSan harness for the scenario-table reader (ecckd_amd/cli/scenario_table.hpp), which bin/ckdmip_lw, bin/ckdmip_sw,
// bin/lw_spectra and bin/sw_spectra share: a well-formed table with comments, blank lines, tabs, a last line without a newline
// and every kind of SPEC; then every refusal of the grammar - a missing file, an empty table, too few and too many SPECs (the
// line is named), an unknown SPEC, `scale=` without a number, a number with a tail, a duplicate output - each by its message.
// The header needs nothing of the library but the error code, so the program links against nothing.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 tools/check_scenario_table.cpp \
//        -o /tmp/check_scenario_table && /tmp/check_scenario_table
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../ecckd_amd/cli/scenario_table.hpp"

using namespace tool;

#define REQUIRE(cond)                                                                           \
  do {                                                                                          \
    if (!(cond)) { std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static std::vector<std::string> written;

static std::string write_table(const std::string& text) {
  static int n = 0;
  const char* tmp = std::getenv("TMPDIR");
  const std::string path = std::string(tmp ? tmp : "/tmp") + "/check_scenario_table_" + std::to_string(++n) + ".txt";
  std::ofstream(path) << text;
  written.push_back(path);
  return path;
}

// the message of the refusal, or "" when the table is accepted
static std::string refusal(const std::string& path, size_t ngas) {
  try {
    read_scenarios(path, ngas);
  } catch (const Fatal& f) {
    REQUIRE(f.code == ECCKD_PARAMETER_ERROR);
    return f.msg;
  }
  return "";
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
  const std::string good = write_table("# a comment\n\n  base\tbase.nc asis asis   asis # trailing\n"
                                       "half half.nc scale=0.5 conc=3e-4 const=1e-6\n\t\n"
                                       "last last.nc scale=-1 asis scale=1e3");
  const std::vector<ScenarioRow> rows = read_scenarios(good, 3);
  REQUIRE(rows.size() == 3 && rows[0].name == "base" && rows[0].output == "base.nc" && rows[2].output == "last.nc");
  for (const GasArg& a : rows[0].specs) REQUIRE(a.mode == GasArg::NONE && a.value == 1.0 && a.path.empty());
  REQUIRE(rows[1].specs[0].mode == GasArg::SCALE && rows[1].specs[0].value == 0.5);
  REQUIRE(rows[1].specs[1].mode == GasArg::CONC && rows[1].specs[1].value == 3e-4);
  REQUIRE(rows[1].specs[2].mode == GasArg::CONST && rows[1].specs[2].value == 1e-6);
  REQUIRE(rows[2].specs[0].value == -1.0 && rows[2].specs[2].value == 1e3);
  REQUIRE(read_scenarios(write_table("only only.nc\n"), 0).size() == 1);                 // no spectrum file, no SPEC

  REQUIRE(has(refusal("/nonexistent/table.txt", 3), "Cannot open scenario table"));
  REQUIRE(has(refusal(write_table(""), 3), "is empty"));
  REQUIRE(has(refusal(write_table("# nothing\n\n   \n"), 3), "is empty"));
  REQUIRE(has(refusal(write_table("a a.nc asis asis asis\nb b.nc asis\n"), 3), ".txt:2: 1 scaling spec(s) for 3 spectrum file(s)"));
  REQUIRE(has(refusal(write_table("a a.nc asis asis asis asis\n"), 3), ".txt:1: 4 scaling spec(s) for 3"));
  REQUIRE(has(refusal(write_table("lonely\n"), 3), ".txt:1: 0 scaling spec(s)"));
  REQUIRE(has(refusal(write_table("a a.nc asis double=2 asis\n"), 3), "unknown scaling spec \"double=2\""));
  REQUIRE(has(refusal(write_table("a a.nc asis ASIS asis\n"), 3), "unknown scaling spec \"ASIS\""));
  REQUIRE(has(refusal(write_table("a a.nc asis scale= asis\n"), 3), "no number after '='"));
  REQUIRE(has(refusal(write_table("a a.nc asis conc=1e-4x asis\n"), 3), "no number after '='"));
  REQUIRE(has(refusal(write_table("a a.nc asis =2 asis\n"), 3), "unknown scaling spec \"=2\""));
  REQUIRE(has(refusal(write_table("a a.nc asis asis asis\n\n# x\nb a.nc scale=2 asis asis\n"), 3), ".txt:4: duplicate output file \"a.nc\""));
  for (const std::string& path : written) std::remove(path.c_str());
  std::printf("check_scenario_table: ok\n");
  return 0;
}
