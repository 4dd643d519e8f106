// What tghip_query_vertex decides about a call before anything touches the device: the refusals of a malformed description, of missing, unwanted or
// misaligned arrays, of a batch past 2^31 - 1 paths and of a start medium the uploaded scene does not have.  Plain host arithmetic over
// TgHipVertexQueryDesc, the pointers' values -- nothing is read through them -- and a few facts of the scene: no device, no context
// (include/tungsten_host.h: tgh_query_vertex_check runs it on its own).
#ifndef TGAMD_VERTEXQUERY_HPP_
#define TGAMD_VERTEXQUERY_HPP_

#include "../../../include/tungsten_host.h"

#include <cstddef>
#include <string>

// TGHIP_OK or TGHIP_E_INVALID with the refusal in `error`.  scene: see TgHostVertexScene; nullptr = no media.
int checkVertexQuery(const TgHipVertexQueryDesc *desc, const void *rays, const void *media, const void *paths, const void *alive, size_t n,
                     const TgHostVertexScene *scene, std::string &error);

#endif
