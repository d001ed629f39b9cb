// `compute potential/atom` on the device (conp_potatom.hip): the pair launch and the finishing launch of
// conp_potential_atom_device.  The k-space part between them belongs to the provider (EwaldQuery / PppmMesh ::potential_device).
// Nothing here allocates once the buffers have their sizes, copies to the host or synchronises.
#include "conp_potatomstyle.hpp"

namespace conp {
using namespace dev;

void PotentialAtom::pair_part(const PotPairArgs &a, const TransposedView &tv) {
  if (!a.numneigh || !a.first || !a.x || !a.q || !a.type || !a.flags || !a.cutsq || !a.pot || !tv.own_row || !tv.tr_ptr ||
      a.ntotal > tv.nall)
    throw ConpError(CONP_ERR_ARG, "conp_potential_atom_device: null array in the pair part");           // (never a launch on a null pointer)
  ctx.prof.begin("potatom_pair", ctx.stream);
  launch_pot_pair(ctx.stream, a, tv);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void PotentialAtom::finish(PotFinishArgs a, int nlocal) {
  if (a.nt > 0 && (!a.targets || !a.x || !a.q || !a.pot || (a.eta != 0.0 && !a.flags)))
    throw ConpError(CONP_ERR_ARG, "conp_potential_atom_device: null array in the finishing step");      // (never a launch on a null pointer)
  if (a.slab) {
    kspace_four_sums(ctx, d_kf_sums, nlocal, a.x, a.q);      // fixed order, on the device
    a.four = d_kf_sums.p;
  }
  a.u = d_u.p;
  ctx.prof.begin("potatom_finish", ctx.stream);
  launch_pot_finish(ctx.stream, a);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
