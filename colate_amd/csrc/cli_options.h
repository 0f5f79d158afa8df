// colate_amd/csrc/cli_options.h -- the parsed command line of `Colate` and `CoalRate`, and what every mode says at its end or after
// a failed library call (mut_driver.cpp).
#pragma once
#include <map>
#include <string>

namespace colate_drv {

struct Options {
  std::map<std::string, std::string> kv;
  bool has(const std::string& k) const { return kv.count(k) > 0; }
  const std::string& get(const std::string& k) const { return kv.at(k); }
  // the option's text through std::stoi / std::stof, as the reference reads its numbers (--years_per_gen is a float there); text
  // that is no number throws, and colate_mut_main prints "Error: <what()>"
  int get_int(const std::string& k) const { return std::stoi(get(k)); }
  float get_float(const std::string& k) const { return std::stof(get(k)); }
};

void print_help();          // the option list
void print_usage_footer();  // "CPU Time spent: ...; Max Memory usage: ..." (coal.cpp:3852-3861)
int api_error(int rc);      // a failed C-ABI call: "Error: <the library's message> (<rc>)"; returns the exit code

}  // namespace colate_drv
