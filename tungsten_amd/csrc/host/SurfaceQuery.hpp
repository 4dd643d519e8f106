// What tghip_query_surface decides about a call before anything touches the device: the refusals of a malformed description, of missing or misaligned
// arrays and of a batch past 2^31 - 1 rays.  Plain host arithmetic over TgHipSurfaceQueryDesc and the pointers' values -- nothing is read through
// them --: no device, no context (include/tungsten_host.h: tgh_query_surface_check runs it on its own).
#ifndef TGAMD_SURFACEQUERY_HPP_
#define TGAMD_SURFACEQUERY_HPP_

#include "../../../include/tungsten_hip.h"

#include <cstddef>
#include <string>

// TGHIP_OK, or TGHIP_E_INVALID with the refusal in `error`
int checkSurfaceQuery(const TgHipSurfaceQueryDesc *desc, const void *rays, const void *out, size_t n, std::string &error);

#endif
