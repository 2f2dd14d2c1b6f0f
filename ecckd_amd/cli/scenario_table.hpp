// scenario_table.hpp - the text table of `ckdmip_lw / ckdmip_sw --scenarios` and of `lw_spectra / sw_spectra scenarios=`: `#` starts a
// comment, blank lines are skipped, one line per scenario,  NAME OUTPUT SPEC_1 ... SPEC_n,  exactly one SPEC per spectrum file
// in the order the tool was given them, a SPEC one of  asis  scale=S  conc=C  const=C.  One grammar, read here; what a SPEC
// means to a tool, and whether it takes const=, is the tool's business.
#pragma once
#include <fstream>
#include <sstream>

#include "tool.hpp"

namespace tool {

struct GasArg {
  std::string path;
  enum { NONE, SCALE, CONC, CONST } mode = NONE;
  double value = 1.0;
};

// One line of a scenario table: the scenario's name, its output file and one GasArg (path empty) per spectrum file
struct ScenarioRow {
  std::string name, output;
  std::vector<GasArg> specs;
};

inline std::vector<ScenarioRow> read_scenarios(const std::string& path, size_t ngas) {
  std::ifstream in(path);
  if (!in) fail(ECCKD_PARAMETER_ERROR, "Cannot open scenario table %s", path.c_str());
  std::vector<ScenarioRow> rows;
  std::string line;
  int lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    const size_t c = line.find('#');
    if (c != std::string::npos) line.erase(c);
    std::istringstream ss(line);
    std::vector<std::string> tok;
    for (std::string t; ss >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    if (tok.size() != 2 + ngas)
      fail(ECCKD_PARAMETER_ERROR, "%s:%d: %zu scaling spec(s) for %zu spectrum file(s) (NAME OUTPUT and one spec per file)", path.c_str(),
           lineno, tok.size() >= 2 ? tok.size() - 2 : (size_t)0, ngas);
    ScenarioRow row;
    row.name = tok[0]; row.output = tok[1];
    for (size_t g = 0; g < ngas; ++g) {
      const std::string& t = tok[2 + g];
      GasArg a;
      const size_t eq = t.find('=');
      const std::string key = t.substr(0, eq);
      if (t == "asis") a.mode = GasArg::NONE;
      else if (eq != std::string::npos && key == "scale") a.mode = GasArg::SCALE;
      else if (eq != std::string::npos && key == "conc") a.mode = GasArg::CONC;
      else if (eq != std::string::npos && key == "const") a.mode = GasArg::CONST;
      else fail(ECCKD_PARAMETER_ERROR, "%s:%d: unknown scaling spec \"%s\" (asis, scale=S, conc=C or const=C)", path.c_str(), lineno, t.c_str());
      if (a.mode != GasArg::NONE) {
        const std::string v = t.substr(eq + 1);
        char* end = nullptr;
        a.value = std::strtod(v.c_str(), &end);
        if (v.empty() || *end) fail(ECCKD_PARAMETER_ERROR, "%s:%d: unknown scaling spec \"%s\" (no number after '=')", path.c_str(), lineno, t.c_str());
      }
      row.specs.push_back(a);
    }
    for (const ScenarioRow& r : rows)
      if (r.output == row.output) fail(ECCKD_PARAMETER_ERROR, "%s:%d: duplicate output file \"%s\"", path.c_str(), lineno, row.output.c_str());
    rows.push_back(row);
  }
  if (rows.empty()) fail(ECCKD_PARAMETER_ERROR, "Scenario table %s is empty", path.c_str());
  return rows;
}

}  // namespace tool
