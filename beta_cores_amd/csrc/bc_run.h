// The protocol of a chunked device run -- _begin, then (_chunk_begin, _chunk_end) until the run's length is reached, then _end --
// as one state and the decisions on it, for bc_viopt.hip, bc_hmc.hip, bc_hmc_small.hip and bc_psvi_many.hip.  Host only: what
// waits for the device is beside bc_run_clock in bc_internal.h / bc_core.hip.
#pragma once
#include <stdint.h>
#include "../../include/beta_cores.h"

void bc_set_error(const char* fmt, ...);

struct bc_run_state {
  bool active = false;             // between _begin and _end
  bool chunk_pending = false;      // something of a chunk is enqueued and has not been waited for
  bool failed = false;             // set by the unit (a mark read at _chunk_end, a refusal that spoils the run): only _end is left
  int64_t done = 0, total = 0;     // steps (iterations) enqueued so far, and the run's length
};

// how a kind of run is named in its messages: `name`_chunk_begin, `name`_chunk_end, `name`_end; `noun`: "steps" or "iterations"
struct bc_run_kind {
  const char *name, *noun;
};

// the tail of every _begin: a fresh run of `total`
static inline void bc_run_open(bc_run_state* r, int64_t total) {
  *r = bc_run_state();
  r->active = true;
  r->total = total;
}

// _chunk_begin: may a chunk of k be admitted?  r: the context's run, or null where none was ever begun; args_ok: the entry
// point's own pointer arguments are there
static inline int bc_run_admit(const bc_run_state* r, const bc_run_kind& kd, bool args_ok, int32_t k) {
  const char* n = kd.name;
  if (!r || !r->active || !args_ok || k <= 0) return bc_set_error("%s_chunk_begin: bad argument, or no run is open", n), BC_INVALID_ARGUMENT;
  if (r->chunk_pending) return bc_set_error("%s_chunk_begin: a chunk is pending (call %s_chunk_end first)", n, n), BC_INVALID_ARGUMENT;
  if (r->failed) return bc_set_error("%s_chunk_begin: the run has failed (call %s_end)", n, n), BC_INVALID_ARGUMENT;
  if (r->done + (int64_t)k <= r->total) return BC_OK;
  bc_set_error("%s_chunk_begin: %d %s after %lld exceed the run's %lld", n, k, kd.noun, (long long)r->done, (long long)r->total);
  return BC_INVALID_ARGUMENT;
}

// _chunk_end (`who`: the entry point, of which bc_hmc_small has two): is a chunk pending to be ended?
static inline int bc_run_pending(const bc_run_state* r, const char* who) {
  return r && r->active && r->chunk_pending ? BC_OK : (bc_set_error("%s: no chunk is pending", who), BC_INVALID_ARGUMENT);
}

// _end: closes the run, if one is open.  *was_pending: a chunk was (abandoned: the caller waits for it, and hands no results out)
static inline int bc_run_close(bc_run_state* r, const bc_run_kind& kd, bool* was_pending) {
  if (!r || !r->active) return bc_set_error("%s_end: no run is open", kd.name), BC_INVALID_ARGUMENT;
  *was_pending = r->chunk_pending;
  r->active = r->chunk_pending = false;
  return BC_OK;
}

// _end, the run closed: may its results be fetched?  `none`: what the caller is left without ("no weights")
static inline int bc_run_complete(const bc_run_state* r, const bc_run_kind& kd, bool was_pending, const char* none) {
  if (!r->failed && !was_pending && r->done == r->total) return BC_OK;
  bc_set_error("%s_end: the run is not complete (%lld of %lld %s%s): %s", kd.name, (long long)r->done, (long long)r->total, kd.noun,
               r->failed ? ", failed" : "", none);
  return BC_INVALID_ARGUMENT;
}
