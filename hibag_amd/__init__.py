"""hibag_amd -- MI355X-native implementation of HIBAG's attribute-bagging
prediction hot path (haplotype-pair posterior loop) behind the reference's own
interface: ``hlaSetKernelTarget("hip")``, ``hlaModelFromObj``, ``hlaPredict``.

The compute lives in ``csrc/libhibag_hip.so`` (hand-written HIP for gfx950,
C ABI in ``include/hibag_hip.h``); there is no CPU fallback in this package.
"""

from .model import (NA_INTEGER, Classifier, HlaAttrBagObj, HlaSNPGeno, engine_kind, engine_nkb, engine_steps, load_geno, load_model, load_model_list,  # noqa: F401
                    model_to_robj, save_model)
from .hibag import (HlaAlleleClass, HlaAttrBagClass, hlaClose, hlaModelFromObj, hlaModelToObj,   # noqa: F401
                    hlaPredict, hlaSetKernelTarget)
from .snpmatch import hlaGenoSwitchStrand, hlaSNPID  # noqa: F401
from .bed import HlaBEDGeno, hlaBED2Geno, hlaLociInfo  # noqa: F401
from .train import (RRandom, hlaAllele, hlaAttrBagging, hlaConcurrentAttrBagging, hlaParallelAttrBagging,  # noqa: F401
                    hlaUniqueAllele, set_seed)
from .merge import hlaAlleleDigit, hlaPredMerge  # noqa: F401
from .predmerge import hlaPredictMerge  # noqa: F401
from .evaluate import (hlaAlleleSubset, hlaCompareAllele, hlaFlankingSNP, hlaGenoSubset, hlaSplitAllele,  # noqa: F401
                       r_sample)
from .oob import hlaOutOfBag  # noqa: F401
from .oobens import hlaOutOfBagEnsemble, out_of_bag_mask  # noqa: F401
from .importance import HlaSNPImportance, hlaSNPImportance  # noqa: F401
from .ld import hlaGenoLD, hlaLDMatrix  # noqa: F401
from .distance import hlaDistance  # noqa: F401
from .submodel import hlaCombineModelObj, hlaSubModelObj  # noqa: F401
from .curve import HlaPredictCurve, hlaPredictCurve  # noqa: F401
from .topk import HlaTopCalls, hlaPredictTopK  # noqa: F401
from .cohort import HlaDeviceCohort, hlaPredictLoci  # noqa: F401
from .draws import HlaPosteriorDraws, hlaPredictDraws  # noqa: F401
from .groups import (HlaAlleleGroups, HlaGroupCalls, hlaGroupsByMap, hlaGroupsByResolution, hlaGroupsBySequence,  # noqa: F401
                     hlaPredictGroups)
from .given import (HlaAlleleConstraint, HlaGivenCalls, hlaConstraintFromAllele, hlaConstraintFromSets,  # noqa: F401
                    hlaPredictGiven)
from .family import (HlaFamilyCalls, HlaMendelCheck, HlaPedigree, hlaMendelCheck, hlaModelAllelePrior,  # noqa: F401
                     hlaPedigreeFromFam, hlaPredictFamily)
from .assoc import HlaAssocResult, hlaAssocTest  # noqa: F401
from .assocglm import HlaAssocGlmResult, hlaAssocGlm  # noqa: F401
from .assocquant import HlaAssocQuantResult, hlaAssocQuant  # noqa: F401
from .assocomni import HlaAssocOmnibusResult, HlaAssocStepwiseResult, hlaAssocOmnibus, hlaAssocStepwise  # noqa: F401
from .associnteract import HlaAssocInteractResult, hlaAssocInteract  # noqa: F401
from .assocscore import HlaAssocScoreResult, hlaAssocScore  # noqa: F401
from .haplo import HlaHaplotypeResult, hlaHaplotypes  # noqa: F401
from .assochaplo import HlaAssocHaploResult, hlaAssocHaplo  # noqa: F401
from .assocsurv import HlaAssocSurvResult, hlaAssocSurv  # noqa: F401
from ._lib import HibagHipError  # noqa: F401

__all__ = ["hlaAssocSurv", "HlaAssocSurvResult", "hlaAssocHaplo", "HlaAssocHaploResult", "hlaHaplotypes", "HlaHaplotypeResult", "hlaAssocScore", "HlaAssocScoreResult","hlaAssocInteract", "HlaAssocInteractResult", "hlaAssocOmnibus", "hlaAssocStepwise", "HlaAssocOmnibusResult", "HlaAssocStepwiseResult", "hlaAssocGlm", "HlaAssocGlmResult", "hlaAssocQuant", "HlaAssocQuantResult", "hlaSNPImportance", "HlaSNPImportance", "engine_kind", "engine_nkb", "engine_steps", "NA_INTEGER", "Classifier", "HlaAttrBagObj", "HlaSNPGeno", "load_geno", "load_model", "model_to_robj", "save_model",
           "HlaAlleleClass", "HlaAttrBagClass", "hlaClose", "hlaModelFromObj", "hlaModelToObj",
           "hlaPredict", "hlaSetKernelTarget", "hlaGenoSwitchStrand", "hlaSNPID", "HibagHipError",
           "HlaBEDGeno", "hlaBED2Geno", "hlaLociInfo", "RRandom", "hlaAllele", "hlaAttrBagging", "hlaConcurrentAttrBagging", "hlaParallelAttrBagging", "hlaUniqueAllele", "hlaAlleleDigit", "hlaPredMerge", "hlaPredictMerge", "hlaAlleleSubset", "hlaCompareAllele", "hlaFlankingSNP", "hlaGenoSubset",
           "hlaSplitAllele", "r_sample", "hlaOutOfBag", "hlaOutOfBagEnsemble", "out_of_bag_mask", "hlaGenoLD", "hlaLDMatrix", "hlaDistance",
           "hlaSubModelObj", "hlaCombineModelObj", "hlaPredictCurve", "HlaPredictCurve", "hlaPredictTopK", "HlaTopCalls",
           "HlaDeviceCohort", "hlaPredictLoci", "load_model_list", "hlaPredictDraws", "HlaPosteriorDraws",
           "HlaAlleleConstraint", "HlaGivenCalls", "hlaConstraintFromAllele", "hlaConstraintFromSets", "hlaPredictGiven",
           "HlaFamilyCalls", "HlaMendelCheck", "HlaPedigree", "hlaMendelCheck", "hlaModelAllelePrior", "hlaPedigreeFromFam",
           "hlaPredictFamily", "HlaAssocResult", "hlaAssocTest",
           "set_seed"]
