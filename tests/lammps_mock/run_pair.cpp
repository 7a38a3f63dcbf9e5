// Driver of the runnable LAMMPS mock (see lmp_mock_core.h): what LAMMPS does around a pair style on one rank --
//   read a structure; pair_style <args>; pair_coeff <args>; init_style; init_one -> neighbor cutoff; periodic ghost images and a
//   FULL neighbor list (cutoff + skin, rotated ilist); compute(eflag, vflag); fold the ghost forces onto their owners (newton on)
// -- with the real pair style classes of lammps/pair_e3gnn_hip.cpp and lammps/pair_d3_hip.cpp linked against libsnet_hip.so.
//   run_pair <e3gnn|e3gnn/parallel|d3> <structure.txt> <out.json> [--steps N] [--empty] [--script FILE] [style args ...] -- <pair_coeff args ...>
// structure.txt:  natoms ntypes / 3 cell rows / skin / natoms x (type x y z)     (cell rows a, b, c; LAMMPS' restricted form for d3)
// Without --script: ONE `run 0` (all flags on, one list, positions fixed).
//   Output JSON: energy, forces[natoms][3] (tag order), virial[6] (LAMMPS order xx yy zz xy xz yz), eatom, counts.
// With --script: a run, one record per step:   eflag vflag rebuild perm_seed ghost_margin / natoms x (x y z), rows in tag order
//   every step     the owned positions are set from the record and every ghost to its owner plus its lattice shift (what
//                  comm->forward_comm() of x does); f is zeroed; compute(eflag, vflag); ghost forces are folded onto their owners
//   rebuild = 1    neighbor.ago = 0; the owned atoms are permuted by perm_seed (0: tag order; tags, types and positions travel
//                  with them), ghost images and the FULL list are regenerated at cutoff + skin + ghost_margin (the margin stands
//                  for the fluctuation of the ghost count in a real run), ilist is rotated by a step-dependent offset, and
//                  atom->x / f / type / tag are reallocated when nall changed.  The first record must rebuild.
//   rebuild = 0    neighbor.ago counts up.  A script in which an owned atom has moved more than skin / 2 since the last rebuild
//                  is refused (exit 4): a skinned list that misses a pair would be the script's mistake, not the pair style's.
//   Around every compute the driver snapshots eng_vdwl, virial and the eatom / vatom arrays, reads the pair's flag members and
//   checks the guard bands behind eatom / vatom (pair.h: PairProbe); a broken band ends the run with exit 5.
//   Output JSON: volume, nlocal, neigh_flags, cutneigh and `steps`: per step eflag, vflag, rebuild, ago, nall, energy, virial,
//   forces / eatom / vatom by tag (eatom / vatom null unless the step asked for them), flags (eflag_either, eflag_global,
//   eflag_atom, vflag_either, vflag_global, vflag_atom, evflag, vflag_fdotr), guard_ok, accum_changed, eatom_changed, vatom_changed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "pair.h"
#include "../../lammps/pair_d3_hip.h"
#include "../../lammps/pair_e3gnn_hip.h"

using namespace LAMMPS_NS;

namespace {
struct Vec3 { double v[3]; };

struct Record {   // one step of a script
  int eflag = 0, vflag = 0, rebuild = 0;
  unsigned perm_seed = 0;
  double ghost_margin = 0.0;
  std::vector<Vec3> pos;   // tag order
};

// everything LAMMPS holds between two neighbor-list rebuilds: local order, ghost images, the FULL list
struct Box {
  int natoms = 0;
  double cell[3][3];
  std::vector<int> type0;                // by tag - 1
  std::vector<int> order;                // local index -> tag - 1
  std::vector<Vec3> xs;                  // [nall]
  std::vector<int> types, tags, owner;   // [nall], [nall], [nghost]: ghost k is an image of local atom owner[k] ...
  std::vector<int> image;                // ... shifted by image[3k .. 3k+3) lattice vectors
  std::vector<int> ilist, numneigh;
  std::vector<std::vector<int>> rows;
  std::vector<int *> first;
  double volume = 0.0;
  int allocated = 0;                     // atoms the Atom arrays were created for

  Vec3 shifted(const Vec3 &p, int sx, int sy, int sz) const {
    Vec3 q;
    for (int d = 0; d < 3; ++d) q.v[d] = p.v[d] + sx * cell[0][d] + sy * cell[1][d] + sz * cell[2][d];
    return q;
  }

  // periodic ghost images within `cut` of any owned atom (what comm->borders() leaves behind), tags = the owners'; then the FULL
  // neighbor list of the owned atoms, ilist rotated by `rot` (a pair style must not assume ilist[ii] == ii)
  void rebuild(const std::vector<Vec3> &pos_by_tag, double cut, int rot) {
    std::vector<Vec3> pos(natoms);
    for (int i = 0; i < natoms; ++i) pos[i] = pos_by_tag[order[i]];
    double vol = cell[0][0] * (cell[1][1] * cell[2][2] - cell[1][2] * cell[2][1]) - cell[0][1] * (cell[1][0] * cell[2][2] - cell[1][2] * cell[2][0]) +
                 cell[0][2] * (cell[1][0] * cell[2][1] - cell[1][1] * cell[2][0]);
    vol = std::fabs(vol);
    volume = vol;
    int reach[3];
    for (int k = 0; k < 3; ++k) {
      const double *a = cell[(k + 1) % 3], *b = cell[(k + 2) % 3];
      const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
      const double height = vol / std::sqrt(cx * cx + cy * cy + cz * cz);
      reach[k] = cut > 0 ? (int)std::ceil(cut / height) : 0;
    }
    xs = pos;
    types.resize(natoms); tags.resize(natoms);
    owner.clear(); image.clear();
    for (int i = 0; i < natoms; ++i) { types[i] = type0[order[i]]; tags[i] = order[i] + 1; }
    for (int sx = -reach[0]; sx <= reach[0]; ++sx)
      for (int sy = -reach[1]; sy <= reach[1]; ++sy)
        for (int sz = -reach[2]; sz <= reach[2]; ++sz) {
          if (!sx && !sy && !sz) continue;
          for (int j = 0; j < natoms; ++j) {
            const Vec3 p = shifted(pos[j], sx, sy, sz);
            bool near = false;
            for (int i = 0; i < natoms && !near; ++i) {
              const double dx = p.v[0] - pos[i].v[0], dy = p.v[1] - pos[i].v[1], dz = p.v[2] - pos[i].v[2];
              near = dx * dx + dy * dy + dz * dz < cut * cut;
            }
            if (near) {
              const int type_j = types[j], tag_j = tags[j];
              xs.push_back(p); types.push_back(type_j); tags.push_back(tag_j); owner.push_back(j);
              image.push_back(sx); image.push_back(sy); image.push_back(sz);
            }
          }
        }
    const int nall = (int)xs.size();
    ilist.assign(natoms, 0); numneigh.assign(nall, 0);
    rows.assign(nall, std::vector<int>());
    first.assign(nall, nullptr);
    for (int ii = 0; ii < natoms; ++ii) ilist[ii] = (ii + rot) % natoms;
    for (int i = 0; i < natoms; ++i) {
      for (int j = 0; j < nall; ++j) {
        if (j == i) continue;
        const double dx = xs[j].v[0] - xs[i].v[0], dy = xs[j].v[1] - xs[i].v[1], dz = xs[j].v[2] - xs[i].v[2];
        if (dx * dx + dy * dy + dz * dz < cut * cut) rows[i].push_back(j);
      }
      numneigh[i] = (int)rows[i].size();
      first[i] = rows[i].data();
    }
  }

  // owned positions from a record, ghosts = owner + lattice shift (comm->forward_comm() of x); the list is not touched
  void move(const std::vector<Vec3> &pos_by_tag) {
    for (int i = 0; i < natoms; ++i) xs[i] = pos_by_tag[order[i]];
    for (size_t k = 0; k < owner.size(); ++k) xs[natoms + k] = shifted(xs[owner[k]], image[3 * k], image[3 * k + 1], image[3 * k + 2]);
  }

  // Atom arrays (reallocated when the atom count changed, as LAMMPS' avec->grow does when nmax is exceeded), comm state, the list
  void publish(Memory &memory, Atom &atom, Comm &comm, NeighList &list, bool empty) {
    const int nall = (int)xs.size();
    atom.nghost = nall - natoms;
    if (nall != allocated) {
      memory.destroy(atom.x); memory.destroy(atom.f); memory.destroy(atom.type); memory.destroy(atom.tag);
      memory.create(atom.x, nall, 3, "atom:x");
      memory.create(atom.f, nall, 3, "atom:f");
      memory.create(atom.type, nall, "atom:type");
      memory.create(atom.tag, nall, "atom:tag");
      allocated = nall;
    }
    for (int i = 0; i < nall; ++i) {
      for (int d = 0; d < 3; ++d) atom.x[i][d] = xs[i].v[d];
      atom.type[i] = types[i];
      atom.tag[i] = tags[i];
    }
    comm.first_ghost = natoms;
    comm.ghost_owner = owner;
    list.inum = empty ? 0 : natoms;
    list.ilist = ilist.data(); list.numneigh = numneigh.data(); list.firstneigh = first.data();
  }
};

std::vector<Record> read_script(const char *path, int natoms) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error(std::string("cannot open ") + path);
  std::vector<Record> out;
  Record r;
  while (in >> r.eflag >> r.vflag >> r.rebuild >> r.perm_seed >> r.ghost_margin) {
    r.pos.resize(natoms);
    for (auto &p : r.pos) in >> p.v[0] >> p.v[1] >> p.v[2];
    if (!in) throw std::runtime_error("malformed script: a record needs natoms position rows");
    out.push_back(r);
  }
  if (!in.eof() || out.empty()) throw std::runtime_error("malformed script");
  if (!out[0].rebuild) throw std::runtime_error("malformed script: the first step must rebuild the neighbor list");
  return out;
}

void permute(std::vector<int> &order, unsigned seed) {   // Fisher-Yates over a fixed LCG; seed 0 = tag order
  const int n = (int)order.size();
  for (int i = 0; i < n; ++i) order[i] = i;
  if (seed == 0) return;
  unsigned long long s = seed;
  for (int i = n - 1; i > 0; --i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(order[i], order[(int)((s >> 33) % (unsigned)(i + 1))]);
  }
}

void print_array(FILE *o, const double *v, int n) {
  std::fputc('[', o);
  for (int k = 0; k < n; ++k) std::fprintf(o, "%s%.17g", k ? ", " : "", v[k]);
  std::fputc(']', o);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: run_pair <style> <structure.txt> <out.json> [--steps N] [--empty] [--script FILE] [style args] -- <pair_coeff args>\n");
    return 2;
  }
  const std::string style = argv[1];
  int steps = 1;
  bool empty = false;
  const char *script = nullptr;
  std::vector<char *> sargs, cargs;
  bool after = false;
  for (int i = 4; i < argc; ++i) {
    if (!after && std::strcmp(argv[i], "--") == 0) { after = true; continue; }
    if (!after && std::strcmp(argv[i], "--steps") == 0 && i + 1 < argc) { steps = std::atoi(argv[++i]); continue; }
    if (!after && std::strcmp(argv[i], "--script") == 0 && i + 1 < argc) { script = argv[++i]; continue; }
    if (!after && std::strcmp(argv[i], "--empty") == 0) { empty = true; continue; }
    (after ? cargs : sargs).push_back(argv[i]);
  }
  try {
    std::ifstream in(argv[2]);
    if (!in) throw std::runtime_error(std::string("cannot open ") + argv[2]);
    int natoms = 0, ntypes = 0;
    Box box;
    double (&cell)[3][3] = box.cell;
    double skin = 0.0;
    in >> natoms >> ntypes;
    for (auto &row : cell) in >> row[0] >> row[1] >> row[2];
    in >> skin;
    std::vector<int> type0(natoms);
    std::vector<Vec3> pos(natoms);
    for (int i = 0; i < natoms; ++i) in >> type0[i] >> pos[i].v[0] >> pos[i].v[1] >> pos[i].v[2];
    if (!in) throw std::runtime_error("malformed structure file");
    std::vector<Record> records;
    if (script) records = read_script(script, natoms);

    LAMMPS lmp;
    Memory memory; Error error; Atom atom; Comm comm; Force force; Neighbor neighbor; Domain domain;
    lmp.memory = &memory; lmp.error = &error; lmp.atom = &atom; lmp.comm = &comm; lmp.force = &force;
    lmp.neighbor = &neighbor; lmp.domain = &domain;
    atom.natoms = natoms; atom.nlocal = natoms; atom.ntypes = ntypes;
    domain.xperiodic = domain.yperiodic = domain.zperiodic = 1;
    for (int k = 0; k < 3; ++k) { domain.boxlo[k] = 0.0; domain.boxhi[k] = cell[k][k]; }
    domain.xy = cell[1][0]; domain.xz = cell[2][0]; domain.yz = cell[2][1];

    // the owned atoms exist before any pair command runs (read_data); ghosts are added once the neighbor cutoff is known
    memory.create(atom.x, natoms, 3, "atom:x");
    memory.create(atom.f, natoms, 3, "atom:f");
    memory.create(atom.type, natoms, "atom:type");
    memory.create(atom.tag, natoms, "atom:tag");
    for (int i = 0; i < natoms; ++i) {
      for (int d = 0; d < 3; ++d) atom.x[i][d] = pos[i].v[d];
      atom.type[i] = type0[i];
      atom.tag[i] = i + 1;
    }
    struct AtomArrays {   // freed on every way out, after the pair style is gone
      Memory &memory; Atom &atom;
      ~AtomArrays() { memory.destroy(atom.x); memory.destroy(atom.f); memory.destroy(atom.type); memory.destroy(atom.tag); }
    } atom_arrays{memory, atom};
    std::unique_ptr<Pair> pair;
    if (style == "e3gnn") pair.reset(new PairE3GNNHip(&lmp));
    else if (style == "e3gnn/parallel") pair.reset(new PairE3GNNHipParallel(&lmp));
    else if (style == "d3") pair.reset(new PairD3Hip(&lmp));
    else throw std::runtime_error("unknown pair style " + style);
    pair->settings((int)sargs.size(), sargs.data());
    pair->coeff((int)cargs.size(), cargs.data());
    pair->init_style();
    const double cut = pair->init_one(1, 1) + skin;   // neighbor.cpp: cutneigh = cutforce + skin

    box.natoms = natoms;
    box.type0 = type0;
    box.order.resize(natoms);
    box.allocated = natoms;
    permute(box.order, 0);
    NeighList list;
    pair->list = &list;   // (neighbor->init_pair hands the style its list)
    const int &nghost = atom.nghost;
    const std::vector<int> &owner = box.owner;

    if (!script) {
      box.rebuild(pos, cut, 7);
      box.publish(memory, atom, comm, list, empty);
      const int nall = natoms + nghost;
      const double vol = box.volume;
      double energy = 0.0, vir[6] = {0, 0, 0, 0, 0, 0};
      std::vector<double> eatom_out(natoms, 0.0);
      for (int s = 0; s < steps; ++s) {
        neighbor.ago = s;   // step 0: the list was just rebuilt; later steps reuse it
        for (int i = 0; i < nall; ++i) atom.f[i][0] = atom.f[i][1] = atom.f[i][2] = 0.0;
        const int eflag = style == "e3gnn" ? 3 : 1, vflag = 2;   // global energy + virial; per-atom energy where the style has it
        pair->compute(eflag, vflag);
        for (int k = 0; k < nghost; ++k)   // newton on: comm->reverse_comm() adds every ghost's force to its owner
          for (int d = 0; d < 3; ++d) atom.f[owner[k]][d] += atom.f[natoms + k][d];
        energy = pair->eng_vdwl;
        std::memcpy(vir, pair->virial, sizeof vir);
        if ((eflag & 2) && pair->eatom) for (int i = 0; i < natoms; ++i) eatom_out[i] = pair->eatom[i];
      }
      FILE *o = std::fopen(argv[3], "w");
      if (!o) throw std::runtime_error(std::string("cannot write ") + argv[3]);
      std::fprintf(o, "{\"energy\": %.17g, \"volume\": %.17g, \"nlocal\": %d, \"nghost\": %d, \"neigh_flags\": %d, \"cutneigh\": %.17g,\n \"virial\": [",
                   energy, vol, natoms, atom.nghost, neighbor.requested_flags, cut);
      for (int k = 0; k < 6; ++k) std::fprintf(o, "%s%.17g", k ? ", " : "", vir[k]);
      std::fprintf(o, "],\n \"eatom\": [");
      for (int i = 0; i < natoms; ++i) std::fprintf(o, "%s%.17g", i ? ", " : "", eatom_out[i]);
      std::fprintf(o, "],\n \"forces\": [");
      for (int i = 0; i < natoms; ++i) std::fprintf(o, "%s[%.17g, %.17g, %.17g]", i ? ", " : "", atom.f[i][0], atom.f[i][1], atom.f[i][2]);
      std::fprintf(o, "]}\n");
      std::fclose(o);
      pair.reset();
      return 0;
    }

    // ---- the scripted run
    std::unique_ptr<FILE, int (*)(FILE *)> out_file(std::fopen(argv[3], "w"), std::fclose);
    FILE *o = out_file.get();
    if (!o) throw std::runtime_error(std::string("cannot write ") + argv[3]);
    int rc = 0;
    std::vector<Vec3> at_rebuild;
    std::vector<double> f_tag((size_t)natoms * 3), e_before, v_before;
    for (size_t s = 0; s < records.size() && rc == 0; ++s) {
      const Record &r = records[s];
      if (r.rebuild) {
        neighbor.ago = 0;
        permute(box.order, r.perm_seed);
        box.rebuild(r.pos, cut + r.ghost_margin, (int)((7 + 13 * s) % (size_t)natoms));
        at_rebuild = r.pos;
      } else {
        neighbor.ago += 1;
        for (int i = 0; i < natoms; ++i) {
          double d2 = 0.0;
          for (int d = 0; d < 3; ++d) d2 += (r.pos[i].v[d] - at_rebuild[i].v[d]) * (r.pos[i].v[d] - at_rebuild[i].v[d]);
          if (d2 > 0.25 * skin * skin) {
            std::fprintf(stderr, "script step %zu: atom %d moved more than skin / 2 since the last rebuild\n", s + 1, i + 1);
            rc = 4;
          }
        }
        if (rc) break;
        box.move(r.pos);
      }
      box.publish(memory, atom, comm, list, empty);
      const int nall = natoms + nghost;
      for (int i = 0; i < nall; ++i) atom.f[i][0] = atom.f[i][1] = atom.f[i][2] = 0.0;

      const double eng_before = pair->eng_vdwl;
      double vir_before[6];
      std::memcpy(vir_before, pair->virial, sizeof vir_before);
      const double *eatom_ptr = pair->eatom, *vatom_ptr = pair->vatom ? pair->vatom[0] : nullptr;
      e_before.assign(eatom_ptr, eatom_ptr + (eatom_ptr ? PairProbe::maxeatom(*pair) : 0));
      v_before.assign(vatom_ptr, vatom_ptr + (vatom_ptr ? (size_t)6 * PairProbe::maxvatom(*pair) : 0));

      pair->compute(r.eflag, r.vflag);

      const bool guard_ok = PairProbe::guard_ok(*pair);
      for (int k = 0; k < nghost; ++k)   // newton on: comm->reverse_comm() adds every ghost's force to its owner
        for (int d = 0; d < 3; ++d) atom.f[owner[k]][d] += atom.f[natoms + k][d];
      for (int i = 0; i < natoms; ++i)
        for (int d = 0; d < 3; ++d) f_tag[3 * (size_t)box.order[i] + d] = atom.f[i][d];
      const bool accum_changed = std::memcmp(&eng_before, &pair->eng_vdwl, sizeof(double)) != 0 ||
                                 std::memcmp(vir_before, pair->virial, sizeof vir_before) != 0;
      const double *ea = pair->eatom, *va = pair->vatom ? pair->vatom[0] : nullptr;
      const bool eatom_changed = ea != eatom_ptr || (size_t)(ea ? PairProbe::maxeatom(*pair) : 0) != e_before.size() ||
                                 (ea && std::memcmp(ea, e_before.data(), e_before.size() * sizeof(double)) != 0);
      const bool vatom_changed = va != vatom_ptr || (size_t)(va ? 6 * (size_t)PairProbe::maxvatom(*pair) : 0) != v_before.size() ||
                                 (va && std::memcmp(va, v_before.data(), v_before.size() * sizeof(double)) != 0);
      int flags[8];
      PairProbe::flags(*pair, flags);

      if (s == 0)
        std::fprintf(o, "{\"volume\": %.17g, \"nlocal\": %d, \"neigh_flags\": %d, \"cutneigh\": %.17g,\n \"steps\": [\n", box.volume, natoms,
                     neighbor.requested_flags, cut);
      std::fprintf(o, "%s  {\"eflag\": %d, \"vflag\": %d, \"rebuild\": %d, \"ago\": %d, \"nall\": %d, \"energy\": %.17g, \"virial\": ", s ? ",\n" : "",
                   r.eflag, r.vflag, r.rebuild, neighbor.ago, nall, pair->eng_vdwl);
      print_array(o, pair->virial, 6);
      std::fprintf(o, ",\n   \"flags\": [%d, %d, %d, %d, %d, %d, %d, %d], \"guard_ok\": %s, \"accum_changed\": %s, \"eatom_changed\": %s, \"vatom_changed\": %s,\n   \"forces\": [",
                   flags[0], flags[1], flags[2], flags[3], flags[4], flags[5], flags[6], flags[7], guard_ok ? "true" : "false",
                   accum_changed ? "true" : "false", eatom_changed ? "true" : "false", vatom_changed ? "true" : "false");
      for (int t = 0; t < natoms; ++t) { if (t) std::fputs(", ", o); print_array(o, &f_tag[3 * (size_t)t], 3); }
      std::fprintf(o, "],\n   \"eatom\": ");
      if ((r.eflag & 2) && guard_ok && pair->eatom) {
        std::vector<double> by_tag(natoms);
        for (int i = 0; i < natoms; ++i) by_tag[box.order[i]] = pair->eatom[i];
        print_array(o, by_tag.data(), natoms);
      } else {
        std::fputs("null", o);
      }
      std::fprintf(o, ", \"vatom\": ");
      if ((r.vflag & 4) && guard_ok && pair->vatom) {
        std::vector<int> local_of(natoms);
        for (int i = 0; i < natoms; ++i) local_of[box.order[i]] = i;
        std::fputc('[', o);
        for (int t = 0; t < natoms; ++t) { if (t) std::fputs(", ", o); print_array(o, pair->vatom[local_of[t]], 6); }
        std::fputc(']', o);
      } else {
        std::fputs("null", o);
      }
      std::fputc('}', o);
      if (!guard_ok) {
        std::fprintf(stderr, "script step %zu: the guard band behind eatom / vatom was overwritten\n", s + 1);
        rc = 5;
      }
    }
    std::fprintf(o, "\n]}\n");
    pair.reset();
    return rc;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
