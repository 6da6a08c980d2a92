// P/Invoke surface of libsnappier_hip_frame_digest.so -- one declaration per function of include/snappier_hip_frame_digest.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameDigest
{
    private const string Lib = "snappier_hip_frame_digest";                     // libsnappier_hip_frame_digest.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): CRC-32C of windows of what framed streams kept with their index decode to, from the chunk headers' CRCs
    // (the five dIdx* pointers are the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes, the three dReq* its requests -- dReqStream holds uint;
    //  dDigest holds uint, dDigLen ulong, dStatus int)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_digest_indexed_workspace(uint nreq, ulong edgeCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_digest_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dReqStream, IntPtr dReqOff, IntPtr dReqLen, uint nreq, ulong edgeCap, IntPtr dDigest, IntPtr dDigLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);

    // ---- host arithmetic: the plain CRC-32C of A || B from the plain CRCs of A and B and B's length
    [DllImport(Lib, CallingConvention = Cc)] internal static extern uint snp_crc32c_combine(uint crcA, uint crcB, ulong lenB);
}
