// P/Invoke surface of libsnappier_hip_frame_verify.so -- one declaration per function of include/snappier_hip_frame_verify.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameVerify
{
    private const string Lib = "snappier_hip_frame_verify";                     // libsnappier_hip_frame_verify.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    internal const ulong SnpVerifyNone = ulong.MaxValue;                        // SNP_VERIFY_NONE: first_bad of a stream with no bad row
    internal const int SnpVerifySkipped = -1;                                   // SNP_VERIFY_SKIPPED: row_status of a row that was not looked at

    // ---- batch, device pointers (asynchronous on the context's stream): the streams and their index as
    // NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes them -> dRowStatus (nentries, int), per stream dStatus (int), dNbad,
    // dFirstBad, dBadBytes (ulong) and dFlags (uint); the decoded bytes go into scratchCap bytes inside dWork in rounds; dResult holds 8 values
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_verify_indexed_workspace(uint nstreams, ulong nentries, uint slotBytes, ulong scratchCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_verify_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, uint slotBytes, ulong scratchCap, IntPtr dRowStatus, IntPtr dStatus, IntPtr dNbad, IntPtr dFirstBad, IntPtr dBadBytes, IntPtr dFlags, IntPtr dWork, IntPtr dResult);

    // ---- the row verdicts as recipes in the form NativeMethodsFrameCompose.snp_frame_compose_indexed_batch takes (dSegFirst nout + 1 values,
    // the others maxSegs) over the sources stream s -> s, replica t -> nstreams + t; dPlanStatus (nout, int); dResult holds 4 values
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_repair_plan_workspace(uint nout);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_repair_plan_batch(IntPtr ctx, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, uint nstreams, IntPtr dRowStatus, IntPtr dRepTotal, IntPtr dRepTail, uint nrepStreams, IntPtr dRpStream, IntPtr dRpReplica, uint nout, uint maxSegs, IntPtr dSegFirst, IntPtr dSegStream, IntPtr dSegOff, IntPtr dSegLen, IntPtr dPlanStatus, IntPtr dWork, IntPtr dResult);
}
