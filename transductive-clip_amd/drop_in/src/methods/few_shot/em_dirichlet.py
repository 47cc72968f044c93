"""Few-shot EM-Dirichlet, drop-in for the reference's src/methods/few_shot/em_dirichlet.py."""
from src.methods._em_dirichlet_base import EMDirichletBase, FewShotMixin


class BASE(FewShotMixin, EMDirichletBase):
    FEW_SHOT = True
    IN_PLACE_FEATURES = ("softmax",)


class EM_DIRICHLET(BASE):
    HARD = False
    BANNER = "EM-DIRICHLET"
