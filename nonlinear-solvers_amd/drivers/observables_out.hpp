// observables_out.hpp -- the drivers' opt-in observables file: with NLS_OBSERVABLES=<path>
// in the environment a driver also writes one nls_observables row per stored snapshot
// (float64 [num_snapshots, NLS_OBS_NFIELDS], include/nls.h) to that path.  Argv, stdout,
// exit codes and the trajectory file are the same with and without it.
#pragma once
#include <cstdlib>
#include <vector>

#include "nls.h"
#include "npy.hpp"

namespace nls {

inline const char *observables_path() {
  const char *p = std::getenv("NLS_OBSERVABLES");
  return p && *p ? p : nullptr;
}

inline void write_observables(const char *path, const std::vector<nls_observables> &rows) {
  npy::Writer w = npy::Writer::open<double>(path, {(uint64_t)rows.size(), (uint64_t)NLS_OBS_NFIELDS});
  if (!rows.empty()) w.append(rows.data(), rows.size() * sizeof(nls_observables));
  w.close();
}

}  // namespace nls
