// Recording stand-in for libsnet_hip.so and the HIP runtime, for tests/test_lammps_sequence_cpu.py: every C-ABI function that
// lammps/pair_e3gnn_hip.cpp and lammps/pair_d3_hip.cpp call, with no GPU behind it.  Each call is appended to the file named by
// the environment variable SNET_STUB_LOG as one JSON line (scalar arguments, and which pointers are null), so that a test can
// check WHAT the glue asks the library for on every step of a run.  The functions that return results honour the headers'
// contracts with fixed values: snet_md_compute ADDS 0.5 to f[0 .. 3 nall), 1.0 to *eng, k + 1 to virial[k] if vflag, 0.125 to
// eatom[0 .. nall) if eflag_atom and 0.0625 to vatom[0 .. 6 nall) if vflag_atom, after it has read every input array over its
// full documented extent (a stale or short array is then a sanitizer report, not a silent pass).  The model it pretends to hold:
// E3_equivariant_model, species "Hf O", cutoff 4.0 (SNET_STUB_CUTOFF overrides).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "snet_d3_ref.h"
#include "snet_hip.h"

struct snet_model { int loaded; };
struct snet_md_host { bool reuse_next; };
struct snet_halo { int world; };
struct PairD3 {
  int natoms = 0;
  std::vector<double> force;
  double stress[6];
};

namespace {
std::string last_error = "";
int rccl_token = 0, stream_token = 0;

void log_line(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void log_line(const char *fmt, ...) {
  const char *path = std::getenv("SNET_STUB_LOG");
  if (!path) return;
  FILE *f = std::fopen(path, "a");
  if (!f) return;
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(f, fmt, ap);
  va_end(ap);
  std::fputc('\n', f);
  std::fclose(f);
}
int null_of(const void *p) { return p == nullptr; }
}  // namespace

extern "C" {
// ---- the four HIP runtime calls of the e3gnn constructor / destructor
hipError_t hipGetDeviceCount(int *count) { *count = 1; log_line("{\"fn\": \"hipGetDeviceCount\"}"); return hipSuccess; }
hipError_t hipSetDevice(int device) { log_line("{\"fn\": \"hipSetDevice\", \"device\": %d}", device); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int flags) {
  *stream = reinterpret_cast<hipStream_t>(&stream_token);
  log_line("{\"fn\": \"hipStreamCreateWithFlags\", \"flags\": %u}", flags);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
  log_line("{\"fn\": \"hipStreamDestroy\", \"stream_null\": %d}", null_of(stream));
  return hipSuccess;
}

// ---- snet_hip.h
int snet_abi_version(void) { return SNET_ABI_VERSION; }
const char *snet_last_error(void) { return last_error.c_str(); }

int snet_model_load(const char *path, snet_model **model) {
  log_line("{\"fn\": \"snet_model_load\", \"path\": \"%s\"}", path);
  *model = new snet_model{1};
  return 0;
}
void snet_model_destroy(snet_model *model) { log_line("{\"fn\": \"snet_model_destroy\"}"); delete model; }
int snet_model_info(const snet_model *, float *cutoff, int32_t *n_species, int32_t *n_layers, int32_t *comm_dims, int32_t max_layers) {
  const char *c = std::getenv("SNET_STUB_CUTOFF");
  if (cutoff) *cutoff = c ? (float)std::atof(c) : 4.0f;
  if (n_species) *n_species = 2;
  if (n_layers) *n_layers = 1;
  for (int t = 0; comm_dims && t < max_layers; ++t) comm_dims[t] = 0;
  log_line("{\"fn\": \"snet_model_info\"}");
  return 0;
}
int snet_model_meta(const snet_model *, const char *key, char *value, int32_t capacity) {
  log_line("{\"fn\": \"snet_model_meta\", \"key\": \"%s\"}", key);
  const char *v = !std::strcmp(key, "model_type") ? "E3_equivariant_model" : !std::strcmp(key, "chemical_symbols_to_index") ? "Hf O" : nullptr;
  if (!v || (int32_t)std::strlen(v) + 1 > capacity) { last_error = std::string("snet_model_meta: no such key ") + key; return 3; }
  std::strcpy(value, v);
  return 0;
}

int snet_rccl_unique_id(void *id128) { std::memset(id128, 7, 128); log_line("{\"fn\": \"snet_rccl_unique_id\"}"); return 0; }
int snet_rccl_comm_create(const void *id128, int32_t world, int32_t rank, void **comm) {
  log_line("{\"fn\": \"snet_rccl_comm_create\", \"world\": %d, \"rank\": %d, \"id_null\": %d}", world, rank, null_of(id128));
  *comm = &rccl_token;
  return 0;
}
void snet_rccl_comm_destroy(void *comm) { log_line("{\"fn\": \"snet_rccl_comm_destroy\", \"comm_null\": %d}", null_of(comm)); }
int snet_halo_create(void *comm, int32_t world, int32_t rank, const int32_t *send_counts, const int32_t *send_idx_host,
                     const int32_t *recv_counts, const int32_t *recv_perm_host, snet_halo **out) {
  long send = 0, recv = 0;
  for (int p = 0; p < world; ++p) { send += send_counts[p]; recv += recv_counts[p]; }
  long check = 0;
  for (long k = 0; k < send; ++k) check += send_idx_host[k];
  for (long k = 0; k < recv; ++k) check += recv_perm_host[k];
  log_line("{\"fn\": \"snet_halo_create\", \"world\": %d, \"rank\": %d, \"send_rows\": %ld, \"recv_rows\": %ld, \"comm_null\": %d, \"check\": %ld}",
           world, rank, send, recv, null_of(comm), check);
  *out = new snet_halo{world};
  return 0;
}
void snet_halo_destroy(snet_halo *halo) { log_line("{\"fn\": \"snet_halo_destroy\"}"); delete halo; }
int snet_model_set_rccl_halo(snet_model *model, snet_halo *halo, int32_t fold_forces) {
  log_line("{\"fn\": \"snet_model_set_rccl_halo\", \"model_null\": %d, \"halo_null\": %d, \"fold_forces\": %d}", null_of(model), null_of(halo), fold_forces);
  return 0;
}

int snet_md_create(snet_model *model, snet_md_host **host) {
  log_line("{\"fn\": \"snet_md_create\", \"model_null\": %d}", null_of(model));
  *host = new snet_md_host{false};
  return 0;
}
void snet_md_destroy(snet_md_host *host) { log_line("{\"fn\": \"snet_md_destroy\"}"); delete host; }
// owned atoms in ilist order, then (ghost_mode 1) one node per tag that no owned atom carries, in first-seen order
int snet_md_nodes(int32_t inum, const int32_t *ilist, int32_t nall, const void *tag, int32_t tag_bytes, int32_t ghost_mode,
                  int32_t *node_to_atom_out, int64_t *n_nodes_out) {
  auto tag_of = [&](int a) -> int64_t {
    return tag_bytes == 4 ? (int64_t) static_cast<const int32_t *>(tag)[a] : static_cast<const int64_t *>(tag)[a];
  };
  std::unordered_set<int64_t> seen;
  int64_t n = 0;
  for (int ii = 0; ii < inum; ++ii) { seen.insert(tag_of(ilist[ii])); node_to_atom_out[n++] = ilist[ii]; }
  if (ghost_mode == 1)
    for (int j = 0; j < nall; ++j)
      if (seen.insert(tag_of(j)).second) node_to_atom_out[n++] = j;
  *n_nodes_out = n;
  log_line("{\"fn\": \"snet_md_nodes\", \"inum\": %d, \"nall\": %d, \"tag_bytes\": %d, \"ghost_mode\": %d, \"n_nodes\": %lld}", inum, nall,
           tag_bytes, ghost_mode, (long long)n);
  return 0;
}
int snet_md_list_unchanged(snet_md_host *host) {
  log_line("{\"fn\": \"snet_md_list_unchanged\", \"host_null\": %d}", null_of(host));
  host->reuse_next = true;
  return 0;
}
int snet_md_compute(snet_md_host *host, int32_t inum, const int32_t *ilist, const int32_t *numneigh, const int32_t *const *firstneigh,
                    int32_t nall, const double *x, const int32_t *type, const void *tag, int32_t tag_bytes, const int32_t *type_map,
                    int32_t ntypes, int32_t ghost_mode, int32_t eflag_atom, int32_t vflag, int32_t vflag_atom, double *f, double *eng,
                    double *virial, double *eatom, double *vatom, int32_t *node_to_atom_out, int64_t *n_nodes_out,
                    int64_t *n_edges_out, void *stream) {
  const int list_unchanged = host->reuse_next;
  host->reuse_next = false;
  log_line("{\"fn\": \"snet_md_compute\", \"inum\": %d, \"nall\": %d, \"tag_bytes\": %d, \"ntypes\": %d, \"ghost_mode\": %d, \"eflag_atom\": %d, "
           "\"vflag\": %d, \"vflag_atom\": %d, \"list_unchanged\": %d, \"f_null\": %d, \"eng_null\": %d, \"virial_null\": %d, \"eatom_null\": %d, "
           "\"vatom_null\": %d, \"node_to_atom_null\": %d, \"stream_null\": %d}",
           inum, nall, tag_bytes, ntypes, ghost_mode, eflag_atom, vflag, vflag_atom, list_unchanged, null_of(f), null_of(eng),
           null_of(virial), null_of(eatom), null_of(vatom), null_of(node_to_atom_out), null_of(stream));
  if (inum <= 0 || nall < inum || !ilist || !numneigh || !firstneigh || !x || !type || !tag || !type_map || !f ||
      (eflag_atom && !eatom) || (vflag && !virial) || (vflag_atom && !vatom) || (ghost_mode == 1 && vflag_atom)) {
    last_error = "snet_md_compute (stub): arguments break the contract of snet_hip.h";
    return 1;
  }
  // read every input over its documented extent
  double sum = 0.0;
  int64_t edges = 0;
  for (int a = 0; a < nall; ++a) {
    sum += x[3 * a] + x[3 * a + 1] + x[3 * a + 2] + type[a];
    sum += tag_bytes == 4 ? (double) static_cast<const int32_t *>(tag)[a] : (double) static_cast<const int64_t *>(tag)[a];
    if (type[a] < 1 || type[a] > ntypes || type_map[type[a]] < 0) { last_error = "snet_md_compute (stub): atom type out of range"; return 1; }
  }
  for (int ii = 0; ii < inum; ++ii) {
    const int i = ilist[ii];
    if (i < 0 || i >= nall) { last_error = "snet_md_compute (stub): ilist entry out of range"; return 1; }
    for (int k = 0; k < numneigh[i]; ++k) {
      const int j = firstneigh[i][k] & 0x3FFFFFFF;
      if (j < 0 || j >= nall) { last_error = "snet_md_compute (stub): neighbor index out of range"; return 1; }
      ++edges;
    }
    if (node_to_atom_out) node_to_atom_out[ii] = i;
  }
  if (sum != sum) { last_error = "snet_md_compute (stub): NaN in the inputs"; return 1; }
  for (int k = 0; k < 3 * nall; ++k) f[k] += 0.5;
  if (eng) *eng += 1.0;
  if (vflag)
    for (int k = 0; k < 6; ++k) virial[k] += k + 1;
  if (eflag_atom)
    for (int a = 0; a < nall; ++a) eatom[a] += 0.125;
  if (vflag_atom)
    for (int k = 0; k < 6 * nall; ++k) vatom[k] += 0.0625;
  if (n_nodes_out) *n_nodes_out = inum;
  if (n_edges_out) *n_edges_out = edges;
  return 0;
}

// ---- snet_d3_ref.h: energy 1.0, force 0.25 per component, stress k + 1
PairD3 *pair_init(void) { log_line("{\"fn\": \"pair_init\"}"); return new PairD3; }
int pair_failed(PairD3 *pair) { return pair == nullptr; }
void pair_set_atom(PairD3 *pair, int natoms, int ntypes, int *type, double *x_flat) {
  double sum = 0.0;
  for (int i = 0; i < natoms; ++i) sum += type[i] + x_flat[3 * i] + x_flat[3 * i + 1] + x_flat[3 * i + 2];
  pair->natoms = natoms;
  log_line("{\"fn\": \"pair_set_atom\", \"natoms\": %d, \"ntypes\": %d, \"finite\": %d}", natoms, ntypes, sum == sum);
}
void pair_set_domain(PairD3 *, int xperiodic, int yperiodic, int zperiodic, double *boxlo, double *boxhi, double xy, double xz, double yz) {
  log_line("{\"fn\": \"pair_set_domain\", \"pbc\": [%d, %d, %d], \"boxlo_null\": %d, \"boxhi_null\": %d, \"tilt\": [%.17g, %.17g, %.17g]}", xperiodic,
           yperiodic, zperiodic, null_of(boxlo), null_of(boxhi), xy, xz, yz);
}
void pair_run_settings(PairD3 *, double rthr, double cnthr, const char *damp_name, const char *func_name) {
  log_line("{\"fn\": \"pair_run_settings\", \"rthr\": %.17g, \"cnthr\": %.17g, \"damping\": \"%s\", \"functional\": \"%s\"}", rthr, cnthr, damp_name, func_name);
}
void pair_run_coeff(PairD3 *, int *atomic_numbers) { log_line("{\"fn\": \"pair_run_coeff\", \"numbers_null\": %d}", null_of(atomic_numbers)); }
void pair_run_compute(PairD3 *pair) {
  pair->force.assign((size_t)pair->natoms * 3, 0.25);
  for (int k = 0; k < 6; ++k) pair->stress[k] = k + 1;
  log_line("{\"fn\": \"pair_run_compute\"}");
}
double pair_get_energy(PairD3 *) { log_line("{\"fn\": \"pair_get_energy\"}"); return 1.0; }
double *pair_get_force(PairD3 *pair) { return pair->force.data(); }
double *pair_get_stress(PairD3 *pair) { return pair->stress; }
void pair_fin(PairD3 *pair) { log_line("{\"fn\": \"pair_fin\"}"); delete pair; }
}  // extern "C"
