"""Few-shot Hard EM-Dirichlet, drop-in for src/methods/few_shot/hard_em_dirichlet.py.
Its logged criterions are identically 0, as in the reference (:233-244 evaluates the criterion
after alpha_old has been refreshed)."""
from src.methods._em_dirichlet_base import EMDirichletBase, FewShotMixin


class BASE(FewShotMixin, EMDirichletBase):
    FEW_SHOT = True
    IN_PLACE_FEATURES = ("softmax",)


class HARD_EM_DIRICHLET(BASE):
    HARD = True
    BANNER = "HARD EM-DIRICHLET"
