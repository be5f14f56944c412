/*
 * HIP-backed Template plugin for GiNGR: a registration algorithm whose correspondence function and observation uncertainty are the
 * USER's (the skeleton of registration/config/Template.scala), with `update` on the MI355X.  NOT COMPILED IN THIS REPOSITORY'S
 * IMAGE (no JVM); see INTEGRATION.md.  Same package as HipCPD.scala, for the same reason (the `private[api]` state updaters).
 *
 * The signature is the reference's TemplateRegistration -- getCorrespondence: State => CorrespondencePairs -- plus the two members a
 * user of the trait overrides, as constructor arguments: getUncertainty (default: identity covariance, Template.scala:50-52) and
 * updateSigma2 (default: unchanged, GingrAlgorithm.scala:256-258).  `update` (GingrAlgorithm.scala:192-254) is overridden: the
 * results of the two functions go to the fitter's pair lists (gingr_fitter_set_pairs / gingr_fitter_set_pairs_cov), ONE native
 * update follows, and updateSigma2(newState) is applied to the device state (gingr_fitter_set_sigma2) when the update committed.
 * Covariances that are exact multiples of the identity go to the isotropic list (one consolidated observation per vertex); the others to
 * the covariance list, which the device sums in its landmark pass -- meant for few pairs -- or, with covariancePass = "gram", to the
 * dense covariance list (gingr_fitter_set_pairs_cov_dense): one consolidated precision per vertex and a 3 x 3-weighted Gram pass over
 * the basis, meant for a covariance per vertex (point-to-plane ICP).  The landmark override of computePosterior
 * (:288-296) happens on the device.  `run`, the Metropolis-Hastings chain, loggers and evaluators are untouched; computePosterior-
 * based callers keep working because getCorrespondence / getUncertainty are the user's own functions.
 */
package gingr.api.registration.config

import breeze.linalg.{DenseMatrix, DenseVector}
import gingr.api._
import gingr.hip.GingrHipNative
import scalismo.common.PointId
import scalismo.statisticalmodel.MultivariateNormalDistribution
import scalismo.utils.Random

class HipTemplateRegistration(
  override val getCorrespondence: TemplateRegistrationState => CorrespondencePairs = (_: TemplateRegistrationState) =>
    CorrespondencePairs.empty(),
  uncertainty: (PointId, TemplateRegistrationState) => MultivariateNormalDistribution = (_: PointId, _: TemplateRegistrationState) =>
    MultivariateNormalDistribution(DenseVector.zeros[Double](3), DenseMatrix.eye[Double](3)),
  sigma2Update: TemplateRegistrationState => Double = (s: TemplateRegistrationState) => s.general.sigma2,
  device: Int = 0,
  covariancePass: String = "landmark"
) extends GingrAlgorithm[TemplateRegistrationState, TemplateConfiguration]
    with AutoCloseable {
  require(covariancePass == "landmark" || covariancePass == "gram", s"covariancePass: $covariancePass; need landmark or gram")
  private val session = new HipSession(device)
  def name = "Template-HIP"

  override val getUncertainty: (PointId, TemplateRegistrationState) => MultivariateNormalDistribution = uncertainty
  override def updateSigma2(current: TemplateRegistrationState): Double = sigma2Update(current)

  override def initializeState(general: GeneralRegistrationState, config: TemplateConfiguration): TemplateRegistrationState =
    TemplateRegistrationState(general, config)

  private def isotropic(c: DenseMatrix[Double]): Boolean =
    c(0, 1) == 0.0 && c(0, 2) == 0.0 && c(1, 0) == 0.0 && c(1, 2) == 0.0 && c(2, 0) == 0.0 && c(2, 1) == 0.0 &&
      c(1, 1) == c(0, 0) && c(2, 2) == c(0, 0)

  // what the fitter holds: the correspondence object and the state its uncertainties were asked for (case classes are immutable:
  // identity is enough); the lists are sent again only when either changes
  private var heldPairs: AnyRef = null
  private var heldState: AnyRef = null
  private var heldCounts: (Int, Int) = (0, 0)

  private def pushPairs(f: Long, current: TemplateRegistrationState): Int = {
    val pairs = getCorrespondence(current)
    if ((pairs eq heldPairs) && (current eq heldState)) return 0
    val withCov = pairs.pairs.map { case (pid, p) => (pid, p, getUncertainty(pid, current).cov) }
    val (iso, full) = withCov.partition(t => isotropic(t._3))
    var rc = 0
    if (iso.nonEmpty || heldCounts._1 > 0)
      rc = GingrHipNative.fitterSetPairs(f, iso.map(_._1.id).toArray, iso.flatMap(t => Seq(t._2.x, t._2.y, t._2.z)).toArray,
        iso.map(_._3(0, 0)).toArray)
    if (rc == 0 && (full.nonEmpty || heldCounts._2 > 0)) {
      val (ids, xyz) = (full.map(_._1.id).toArray, full.flatMap(t => Seq(t._2.x, t._2.y, t._2.z)).toArray)
      val cov9 = full.flatMap(t => for (i <- 0 until 3; j <- 0 until 3) yield t._3(i, j)).toArray
      rc =
        if (covariancePass == "gram") GingrHipNative.fitterSetPairsCovDense(f, ids, xyz, cov9)
        else GingrHipNative.fitterSetPairsCov(f, ids, xyz, cov9)
    }
    if (rc == 0) {
      heldPairs = pairs
      heldState = current
      heldCounts = (iso.size, full.size)
    }
    rc
  }

  override def update(current: TemplateRegistrationState, probabilistic: Boolean)(implicit rnd: Random): TemplateRegistrationState = {
    session.bind(current.general, current.config.useLandmarkCorrespondence)
    var committed = false
    val (alpha, pose, status) = session.updateOnce(
      current.general,
      f => {
        var rc = pushPairs(f, current)
        if (rc == 0)
          rc =
            if (probabilistic) GingrHipNative.fitterUpdatePairsSample(f, Array.fill(current.general.model.rank)(rnd.scalaRandom.nextGaussian()))
            else GingrHipNative.fitterUpdatePairs(f, 1)
        rc
      },
      f => committed = GingrHipNative.fitterLastUpdateError(f) == 0
    )
    val next = current.updateGeneral(HipStateUpdate(current.general, alpha, pose, status))
    if (!committed || status == 3) next
    else {
      // updateSigma2(newState) (:244-246); the device state follows so that a resident state stays the host's
      val s2 = updateSigma2(next)
      if (s2 != next.general.sigma2) session.setSigma2(s2)
      next.updateGeneral(next.general.updateSigma2(s2))
    }
  }

  /** log density of `mesh` under the posterior of `current` (GeneratorWrapperStochastic.scala:42-63), on the device */
  def posteriorLogpdf(current: TemplateRegistrationState, mesh: Array[Double]): Double = {
    session.bind(current.general, current.config.useLandmarkCorrespondence)
    val out = new Array[Double](1)
    session.withState(
      current.general,
      f => {
        val rc = pushPairs(f, current)
        if (rc == 0) GingrHipNative.fitterPosteriorLogpdfPairs(f, mesh, out) else rc
      },
      current.config.useLandmarkCorrespondence
    )
    out(0)
  }

  def retryCounter: Int = session.retryCounter
  override def close(): Unit = session.close()
}
