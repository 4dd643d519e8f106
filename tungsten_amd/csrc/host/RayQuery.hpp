// What tghip_query_rays decides about a call before anything touches the device: the refusals of a malformed description, of missing or misaligned
// arrays and of a batch past 2^31 - 1 rays.  Plain host arithmetic over TgHipRayQueryDesc and the pointers' values -- nothing is read through them --:
// no device, no context (include/tungsten_host.h: tgh_query_rays_check runs it on its own).
#ifndef TGAMD_RAYQUERY_HPP_
#define TGAMD_RAYQUERY_HPP_

#include "../../../include/tungsten_hip.h"

#include <cstddef>
#include <string>

// TGHIP_OK, or TGHIP_E_INVALID with the refusal in `error`
int checkRayQuery(const TgHipRayQueryDesc *desc, const void *rays, const void *out, size_t n, std::string &error);

#endif
